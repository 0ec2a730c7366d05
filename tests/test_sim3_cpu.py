"""CPU tests of the Sim3 RANSAC: the ABI declares and exports it, and the CPU restatement (tests/sim3_ref.cpp) that the GPU parity
tests use recovers the known similarity, counts iterations as SetRansacParameters does, decodes sets by the initializer's rule and
replays a run window by window (its own second opinion)."""

import numpy as np
import pytest

import initializer_build
import sim3_build as B
import sim3_cases as S
import sim3_parity as P
from test_abi_cpu import _exports

NEW = ["orbfe_sim3_solve", "orbfe_sim3_solve_batch_device", "orbfe_sim3_inspect"]


def test_header_declares_and_library_exports_the_solver():
    from orb_slam2_aruco_amd import binding, header
    assert set(NEW) <= set(header.functions), sorted(set(NEW) - set(header.functions))
    assert set(NEW) <= set(binding.SYMBOLS)
    import __graft_entry__
    assert "sim3_solver.hip" in __graft_entry__.HIP_SOURCES
    assert set(NEW) <= _exports(), sorted(set(NEW) - _exports())
    assert binding.SIM3_RESULT_DTYPE == B.RESULT_DTYPE       # the record of orbfe.h, field for field
    fields = [name for name, _, _ in header.records["orbfe_sim3_result"]]
    assert fields == list(B.RESULT_DTYPE.names), fields


def _rot_err(Ra, Rb):
    return np.abs(np.asarray(Ra, np.float64).reshape(3, 3) - np.asarray(Rb, np.float64).reshape(3, 3)).max()


@pytest.mark.parametrize("s,fix", [(1.0, True), (1.0, False), (1.3, False), (0.7, False)])
@pytest.mark.parametrize("N", [40, 100, 1000])
def test_restatement_recovers_the_known_similarity_on_noise_free_data(N, s, fix):
    sc = S.scene(N, s, 0.0, fix, seed=1, noise=0.0)
    r = B.solve(sc, *S.RANSAC, words=S.words(300, N))
    res = r["result"]
    assert res["n"] == N and res["found"] == 0 and res["n_inliers"] == N and res["best"] == 0
    assert _rot_err(res["R12"], sc["R12"]) < 1e-4
    assert abs(res["s12"] - sc["s12"]) < 1e-4 * sc["s12"]
    assert np.abs(res["t12"] - sc["t12"]).max() < 1e-4 * sc["extent"]
    T = res["T12"].reshape(4, 4)
    assert np.array_equal(T[:3, 3], res["t12"]) and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.allclose(T[:3, :3], res["s12"] * res["R12"].reshape(3, 3), rtol=1e-6, atol=1e-7)
    # vbInliers: exactly the kept correspondences, by their index in keyframe 1
    assert np.array_equal(r["inliers12"], sc["good"])
    assert np.array_equal(np.flatnonzero(sc["good"]), r["indices1"])


@pytest.mark.parametrize("c", [c for c in S.CASES if c[0] >= 100 and c[2] <= 0.3], ids=S.case_id)
def test_restatement_finds_the_similarity_under_noise_and_outliers(c):
    sc = S.case_scene(c)
    r = B.solve(sc, *S.ransac_of(c), words=S.case_words(c))
    res = r["result"]
    assert res["found"] >= 0 and res["n_inliers"] > 20
    # a 3-point model from points with a pixel of noise: right to a few degrees, its inliers are true correspondences
    cosang = (np.trace(res["R12"].reshape(3, 3).astype(np.float64).T @ sc["R12"]) - 1) / 2
    assert np.degrees(np.arccos(np.clip(cosang, -1, 1))) < 10.0
    assert (r["inliers12"] & ~sc["good"]).sum() <= 0.1 * r["inliers12"].sum()


@pytest.mark.parametrize("N,want_its,want_no_more", [(20, 1, 1), (40, 35, None), (100, 300, None), (19, None, 1)])
def test_iteration_counts_of_set_ransac_parameters(N, want_its, want_no_more):
    """(0.99, 20, 300) with the float epsilon: N = 20 -> 1 (N == minInliers), 40 -> 35, 100 -> 574 clipped to 300, 19 -> bNoMore."""
    assert int(np.ceil(np.log(1 - 0.99) / np.log(1 - float(np.float32(20) / np.float32(40)) ** 3))) == 35
    assert int(np.ceil(np.log(1 - 0.99) / np.log(1 - float(np.float32(20) / np.float32(100)) ** 3))) == 574
    sc = S.scene(N, 1.3, 0.0, False, seed=2)
    r = B.solve(sc, *S.RANSAC, words=S.words(300, 0))
    res = r["result"]
    assert res["n"] == N
    if want_its is not None:
        assert res["max_iterations"] == want_its
    if N == 19:
        assert res["no_more"] == 1 and res["found"] == -1 and res["best"] == -1 and not r["inliers12"].any()
        assert not r["counts"].any() and not r["sets"].any()      # nothing ran, no word was read
    if N == 20:
        # one iteration, and 20 inliers are not MORE than 20: nothing found, no more
        assert res["no_more"] == 1 and res["found"] == -1 and np.count_nonzero(r["sets"].any(axis=1)) <= 1


@pytest.mark.parametrize("N", [3, 4, 100, 1000])
def test_set_decoding_follows_the_initializers_rule(N):
    """Three words padded to eight decode, by the initializer's restatement, to the same first three indices."""
    w = S.words(200, N)
    w[:3] = [0, 2147483647, 1 << 30]
    got = B.decode_sets(N, w)
    if N >= 8:
        w8 = np.zeros((200, 8), np.int32); w8[:, :3] = w.reshape(-1, 3)
        assert np.array_equal(got, initializer_build.decode_sets(N, w8.reshape(-1))[:, :3])
    assert all(len(set(r)) == 3 for r in got.tolist()) and got.min() >= 0 and got.max() < N
    # the same sets come back from a whole run
    sc = S.scene(N, 1.3, 0.0, False, seed=3)
    r = B.solve(sc, 0.99, min(20, N), 300, words=w[:900] if len(w) >= 900 else np.resize(w, 900))
    k = r["result"]["max_iterations"]
    assert np.array_equal(r["sets"][:k], B.decode_sets(N, np.resize(w, 900))[:k])


@pytest.mark.parametrize("c", [(100, 1.3, 0.6, False), (100, 1.0, 0.3, True), (40, 1.3, 0.3, False), (1000, 0.7, 0.6, False)], ids=S.case_id)
def test_window_replay_equals_one_find(c):
    """iterate(5) sixty times, carrying mnIterations and mnBestInliers, returns the same iteration, inliers and model as find()."""
    sc = S.case_scene(c, seed=4)
    w = S.words(300, 7)
    whole = B.solve(sc, *S.RANSAC, words=w)
    best_in, it, hit = 0, 0, None
    for call in range(60):
        r = B.solve(sc, *S.RANSAC, first=it, n_iterations=5, best_in=best_in, words=w[3 * it:3 * it + 15])
        res = r["result"]
        if res["best"] >= 0:
            best_in = int(res["best_inliers"])
            held = res
        if res["found"] >= 0:
            hit = r
            break
        it = min(it + 5, int(res["max_iterations"]))
        if res["no_more"]:
            break
    W = whole["result"]
    if W["found"] >= 0:
        assert hit is not None
        for f in ("found", "n_inliers", "best", "best_inliers", "s12", "R12", "t12", "T12", "no_more"):
            assert np.array_equal(hit["result"][f], W[f]), f
        assert np.array_equal(hit["inliers12"], whole["inliers12"])
    else:
        assert hit is None and res["no_more"] == 1 and W["no_more"] == 1
        assert best_in == W["best_inliers"] and held["best"] == W["best"] and np.array_equal(held["T12"], W["T12"])


def eigen_gap_ok(eig):
    l1, l2 = eig[:, 0].astype(np.float64), eig[:, 1].astype(np.float64)
    return (l1 - l2) > 0.03 * np.abs(l1)


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_scenes_keep_the_excluded_share_under_the_cap(c):
    """The GPU parity test compares the hypotheses whose N matrix has well separated leading eigenvalues, (l1 - l2) > 0.03 |l1|, and
    caps the excluded share at 15 %: a condition on the scenes, checked here with the restatement's own eigenvalues."""
    sc = S.case_scene(c)
    r = B.solve(sc, *S.ransac_of(c), words=S.case_words(c))
    ran = min(300, int(r["result"]["max_iterations"])) if r["N"] >= max(3, S.ransac_of(c)[1]) else 0
    if ran == 0:
        return
    share = 1.0 - eigen_gap_ok(r["eig"][:ran]).mean()
    print("%s: %d hypotheses, excluded share %.3f" % (S.case_id(c), ran, share))
    assert share <= 0.15


@pytest.mark.parametrize("c", [c for c in S.CASES if c[0] >= 100 and c[2] <= 0.3], ids=S.case_id)
def test_required_cases_have_a_clear_decision(c):
    """The parity contract compares found / n_inliers / best where the restatement's scan is clear, and requires that of the
    outlier-free and 30 % cases at N >= 100: a condition on the scenes and words, checked here."""
    sc = S.case_scene(c)
    prob, min_inl, max_it = S.ransac_of(c)
    want = B.solve(sc, prob, min_inl, max_it, words=S.case_words(c))
    assert P.decision_reason(want, sc, min_inl, max_it) is None
