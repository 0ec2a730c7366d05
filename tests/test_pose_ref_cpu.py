"""The CPU side of the hard marker-pose cases: tests/golden/pose_hard_cases.npz regenerates identically, its 50-digit reference
(tests/pose_ref.py) is held to geometry, and the CPU oracle is held to the reference by the contract of tests/pose_contract.py that
tests/test_pose_gpu.py applies to the device.

Measured here (the generator prints them): the oracle's envelope A = 177 (eR (pi - w)^2 / eps near a half turn, over 2 x 300
fronto-parallel markers and the committed cases; median about 1), B = 9.6e-12 (eR elsewhere); F, the float rounding of the reference's own
rotation vector, 1e-8 .. 1.3e-7; the oracle's translations within 1.6e-11 relative of the reference everywhere.  The plain double
evaluation of the stages, in eps times the stage's condition: homography 0.19, rotations 2.2, translation 1.1, eigenvector 2.1.

NaN: on 6 x 1000 fronto-parallel markers (three seeds, with and without distortion) the oracle gives no record that is NaN in all 14
values, and 3 to 12 of 1000 in which the rotation vector and the error of ONE solution are NaN: the true, half-turn solution, whose trace
rounds below -1 so that rot2vec's acos has no value.  A zero radicand (all 14 NaN) needs the marker on the optical axis as well, which a
random position does not give; two of the four degenerate records show it."""
import functools

import numpy as np
import pytest

import gen_pose_golden as gen
import oracle_lib
import pose_cases as pc
import pose_contract as contract
import pose_hard_cases as hc


@functools.lru_cache(None)
def built():
    return gen.build()


@functools.lru_cache(None)
def fixture():
    return contract.Fixture(gen.PATH)


def oracle_record(fx, i):
    K4, dist, size = fx.camera(i)
    return oracle_lib.marker_pose(fx["corners"][i], np.float32(size), K4, dist)


def test_fixture_regenerates_identically():
    new, old = built(), fixture().d
    assert sorted(new) == sorted(old)
    for k in new:
        a, b = np.asarray(new[k]), old[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    assert 300 <= len(old["fam"]) <= 600 and (np.bincount(old["fam"]) >= 2).all()


def test_families_are_what_they_say():
    fx = fixture()
    names = list(fx["fam_names"])
    assert {"fronto_dist", "fronto_nodist", "near_fronto_0.0001", "near_fronto_0.001", "near_fronto_0.01", "near_fronto_0.05", "steep_1.3", "steep_1.5",
            "pixel_grid", "coef8", "coef12", "behind", "cam_fx_fy", "cam_resized", "size_1e-3", "size_100", "px_1.5", "outside", "degenerate"} <= set(names)
    assert fx["fam_ndist"][names.index("coef8")] == 8 and fx["fam_ndist"][names.index("coef12")] == 12 and (fx["fam_dist"][names.index("coef12")] != 0).all()
    K = fx["fam_K4"]
    assert K[names.index("cam_fx_fy")][1] == 2 * pc.K4[1] and np.array_equal(K[names.index("cam_resized")], oracle_lib.camera_resize(pc.K4, (1280, 720), (640, 480)))
    g = fx["corners"][fx.family("pixel_grid")]
    assert len(g) == 8 and (g == np.rint(g)).all() and np.array_equal(g[0], hc.GRID_SQUARE) and np.array_equal(g[4], hc.GRID_SQUARE + np.float32([37, -21]))
    span = lambda name: np.ptp(fx["corners"][fx.family(name)], axis=1).max(1)
    assert span("px_1.5").max() < 2.5 and span("px_1.5").min() > 0.8
    out = fx["corners"][fx.family("outside")]
    assert out.min() < 0 and out.max() > 640 and out.min() >= -400 and out.max() <= 1000
    assert fx["pimw"][fx.family("behind")].max(1).min() > np.pi - 0.35          # the true rotations are near the identity
    for name in ("fronto_dist", "fronto_nodist"):
        assert fx["pimw"][fx.family(name)].min(1).max() < 1e-3          # one solution of each is the half turn
    d = fx["corners"][fx.family("degenerate")]
    assert (d[0] == d[0][0]).all() and np.array_equal(d[1][0], d[1][1]) and np.array_equal(d[1][2], d[1][3])
    v = d[2] - d[2][0]
    assert (v[1:, 0] * v[1, 1] == v[1:, 1] * v[1, 0]).all()            # collinear, exactly


def test_reference_is_geometry():
    """Both reference rotations are rotations, and the noise-free true pose is one of the two solutions: its translation within
    8 delta / h relative, delta = 2^-24 max |corner| the float rounding of a corner and h = area / longest side the marker's height in the
    image (a corner error of delta moves the scale, hence t, by delta / h; 8 for four corners and two coordinates).  Measured: at most
    2.0 delta / h, in every family, with five, eight, twelve or no coefficients."""
    fx = fixture()
    truth = [(R, t) for f in hc.families() for _, R, t in f["cases"]]
    worst = 0.0
    for i in range(fx.n):
        if not fx["valid"][i]:
            continue
        for k in range(2):
            R = fx["R"][i, k].reshape(3, 3)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14, (i, k)
        if truth[i][0] is not None:
            q = fx["corners"][i].astype(np.float64)
            area = 0.5 * abs((q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1]).sum())
            h = area / np.linalg.norm(np.roll(q, -1, 0) - q, axis=1).max()
            rel = min(np.abs(fx["t"][i, k] - truth[i][1]).max() for k in range(2)) / np.abs(truth[i][1]).max()
            worst = max(worst, rel / (2.0 ** -24 * np.abs(q).max() / h))
            assert rel <= 8 * 2.0 ** -24 * np.abs(q).max() / h, (i, rel)
    print("true translation recovered within %.2f delta / h" % worst)
    assert (fx["rad"][fx["valid"]] >= 0).all() and (fx["rms"][fx["valid"]].min(1) < 1e-3).all()


def test_oracle_holds_the_contract_and_is_inside_its_envelope():
    fx = fixture()
    classes = {}
    for i in range(fx.n):
        cls, eR = contract.check(fx, i, *oracle_record(fx, i), who="oracle")
        classes.setdefault(str(fx["fam_names"][fx["fam"][i]]), []).append(cls)
        for k in range(2):
            if np.isfinite(eR[k]):
                assert eR[k] <= fx["A"] * contract.EPS / fx["pimw"][i, k] ** 2 + fx["B"] if fx["pimw"][i, k] else True, (i, k, eR[k])
    assert np.nanmax(fx["oracle_et"]) < 1e-9
    assert classes.pop("degenerate") == ["all", "all", "none", "none"]
    assert classes.pop("fronto_half_turn") == ["solution", "solution"]
    assert all(c == "none" for v in classes.values() for c in v)
    assert 1 < fx["A"] < 1e4 and fx["B"] < 1e-9 and 0 < np.nanmin(fx["F"]) and np.nanmax(fx["F"]) < 2e-7
    print("A = %.3g, B = %.3g, F = %.3g .. %.3g; W_H %.3g W_rot %.3g W_t %.3g W_ev %.3g" % (
        fx["A"], fx["B"], np.nanmin(fx["F"]), np.nanmax(fx["F"]), fx["W_H"], fx["W_rot"], fx["W_t"], fx["W_ev"]))


def test_oracle_on_the_pixel_grid_squares():
    """The centred square is an exact half turn: R[7] - R[5] is exactly 0, rot2vec returns 0 for both solutions and the reprojection
    through the identity misses by 50 sqrt(2) px.  The shifted square is an ordinary fronto-parallel marker: its exact best solution
    reprojects at 2e-6 px, the oracle's at up to 0.03 px through rot2vec's error (the issue measured up to 4 px on such markers)."""
    fx = fixture()
    idx = fx.family("pixel_grid")
    for i in idx[:4]:
        r1, t1, r2, t2, err = oracle_record(fx, i)
        assert (r1 == 0).all() and (r2 == 0).all() and np.allclose(err, 70.71068, atol=1e-4) and np.allclose(t1, [0, 0, 1], atol=1e-12)
    shifted = [float(oracle_record(fx, i)[4][0]) for i in idx[4:]]
    print("shifted squares: exact best RMS %.2g px, the oracle's err[0] %s" % (fx["rms"][idx[4:]].min(1).max(), shifted))
    assert fx["rms"][idx[4:]].min(1).max() < 1e-4 and max(shifted) < 4.0


@pytest.mark.parametrize("with_dist", [True, False])
def test_oracle_nan_share_on_fronto_parallel_markers(with_dist):
    worst = 0
    for seed in (1, 2, 3):
        c, K4, dist = hc.fronto_sample(1000, seed, with_dist)
        rec = np.array([np.concatenate([np.concatenate(w[:4]), w[4]]) for w in (oracle_lib.marker_pose(x, np.float32(hc.SIZE), K4, dist) for x in c)])
        cls = contract.nan_class(rec)
        assert (cls >= 0).all(), (seed, rec[cls < 0])
        worst = max(worst, int((cls > 0).sum()))
        assert (cls > 0).sum() <= 20, (seed, (cls > 0).sum())            # 2 %
    print("NaN records of 1000, worst seed: %d" % worst)


def test_dropped_coefficients_move_the_pose():
    """the eight- and twelve-coefficient families see their last coefficients: solved with the vector cut to five (to eight), the
    translation moves by far more than the 1e-5 the device is held to"""
    fx = fixture()
    for name, keep in (("coef8", 5), ("coef12", 8)):
        moved = []
        for i in fx.family(name):
            K4, dist, size = fx.camera(i)
            full, cut = oracle_lib.marker_pose(fx["corners"][i], np.float32(size), K4, dist), oracle_lib.marker_pose(fx["corners"][i], np.float32(size), K4, dist[:keep])
            moved.append(np.abs(full[1] - cut[1]).max() / np.abs(full[1]).max())
        print(name, "median relative move of t %.3g" % np.median(moved))
        assert np.median(moved) > 1e-4, (name, np.median(moved))
