"""The cases of tests/match_batch_cases.py are not vacuous: with the oracle alone, every parity case of
tests/test_match_batch_device_gpu.py has matches wherever both sides hold at least 63 keypoints, and every overflow case overflows
the sizes a fresh matcher workspace starts with (row stride 128, 16 384 pool entries per pair, 1024 level-0 keypoints)."""
import numpy as np
import pytest

import match_batch_cases as mc
import oracle_lib as oracle

SEED = 7
FIRST_ROW_STRIDE, FIRST_POOL, MAX_LEVEL0 = 128, 16384, 1024


@pytest.fixture(scope="module")
def rag():
    return mc.ragged_frames(SEED)


def _big(case, f):
    return case["n"][f] >= 63


def test_ragged_frames_layout(rag):
    assert rag["n"].tolist() == mc.COUNTS and rag["capacity"] == 384 and rag["kps"].shape == (8, 384)
    for f, n in enumerate(mc.COUNTS):
        k = rag["kps"][f]
        assert np.all(np.isfinite(k["x"][:n])) and np.all((k["octave"][:n] >= 0) & (k["octave"][:n] <= 7))
        assert np.all(np.isnan(k["x"][n:])) and np.all(k["octave"][n:] == -1) and np.all(rag["desc"][f, n:] == 0xA5)
    assert set(np.unique(rag["kps"][5]["octave"])) == set(range(8))


def test_knn2_pairs_cover_the_edges():
    Q, T = mc.knn2_pairs(SEED)
    nq, nt = [len(q) for q in Q], [len(t) for t in T]
    assert 0 in nq and 0 in nt and {1, 63, 64, 65} <= set(nq) and nq.count(max(nq)) == 1 and nt.count(max(nt)) == 1
    bi, bd, sd = oracle.knn2(Q[5], T[5])
    assert bi[0] == 3 and bd[0] == 0 and sd[0] == 0 and bd[2] == 32 and sd[2] == 32    # the planted ties


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("bounds", [None, mc.DISTORTED_BOUNDS])
def test_search_for_initialization_pairs_have_matches(rag, ori, bounds):
    order = list(range(8)) + [0]                 # the empty frame as F1 of pair 0 and as F2 of pair 7
    case = mc.reorder(rag, order)
    for p in range(8):
        (k1, d1), (k2, d2) = case["frames"][p], case["frames"][p + 1]
        n, m12, _ = oracle.search_for_initialization(k1, d1, k2, d2, mc.COLS, mc.ROWS, None, 100, 0.9, ori, bounds)
        if _big(case, p) and _big(case, p + 1):
            assert n > 0, p
        if len(k1) == 0 or len(k2) == 0:
            assert n == 0


def test_projection_queries_have_matches(rag):
    qs = mc.projection_queries(rag, SEED + 1, 200)
    assert qs["nq"].tolist() == [1, 63, 64, 65, 200, 200, 2, 0]
    for f in range(8):
        k, d = rag["frames"][f]
        m = qs["nq"][f]
        got = oracle.search_by_projection(k, d, mc.COLS, mc.ROWS, qs["q"][f, :m], qs["qdesc"][f, :m], qs["taken"][f, :len(k)], 1, 100, 0.8,
                                          q_observed=qs["qobs"][f, :m])
        if _big(rag, f) and m >= 63:
            assert got["nmatches"] > 0, f
        assert mc.longest_candidate_list(k, qs["q"][f, :m]) <= FIRST_ROW_STRIDE      # the parity test never needs the retry


def test_projection_overflow_case_overflows_only_in_frame_3():
    case, qs = mc.projection_overflow_case(SEED)
    longest = [mc.longest_candidate_list(case["frames"][f][0], qs["q"][f, :qs["nq"][f]]) for f in range(5)]
    assert longest[3] == 600 > FIRST_ROW_STRIDE
    assert all(l <= FIRST_ROW_STRIDE for f, l in enumerate(longest) if f != 3), longest
    k, d = case["frames"][3]
    got = oracle.search_by_projection(k, d, mc.COLS, mc.ROWS, qs["q"][3, :1], qs["qdesc"][3, :1], qs["taken"][3, :600], 1, 100, 0.8)
    assert got["nmatches"] == 1
    # the match sits behind candidate position 128: a row cut at the first stride cannot hold it
    _, order = oracle.features_in_area(k, mc.COLS, mc.ROWS, [320.0], [220.0], 50.0, 0, -1)
    assert order.tolist().index(int(got["match"][0])) >= FIRST_ROW_STRIDE


def test_sfi_overflow_case_overflows_only_in_pair_1():
    case = mc.sfi_overflow_case()
    need = [mc.sfi_candidates(case["frames"][p][0], case["frames"][p + 1][0], 100) for p in range(3)]
    assert need[1] > FIRST_POOL and need[0] <= FIRST_POOL and need[2] <= FIRST_POOL, need
    for p in range(3):
        (k1, d1), (k2, d2) = case["frames"][p], case["frames"][p + 1]
        assert oracle.search_for_initialization(k1, d1, k2, d2, mc.COLS, mc.ROWS, None, 100, 0.9, True)[0] > 0, p


def test_sfi_capacity_case():
    case = mc.sfi_capacity_case()
    l0 = [int((k["octave"] <= 0).sum()) for k, _ in case["frames"]]
    assert l0[2] == 1100 > MAX_LEVEL0 and all(c < MAX_LEVEL0 for f, c in enumerate(l0) if f != 2), l0
    need = [mc.sfi_candidates(case["frames"][p][0], case["frames"][p + 1][0], 10) for p in range(4)]
    assert max(need) < 1100, need                 # the pool flag stays below the level-0 count the status call has to report
    for p in (0, 3):
        (k1, d1), (k2, d2) = case["frames"][p], case["frames"][p + 1]
        assert oracle.search_for_initialization(k1, d1, k2, d2, mc.COLS, mc.ROWS, None, 10, 0.9, True)[0] > 0, p


def test_sfi_capacity_and_pool_case():
    case, follow = mc.sfi_capacity_and_pool_case(), mc.sfi_overflow_case()
    assert int((case["frames"][2][0]["octave"] <= 0).sum()) == 1100 > MAX_LEVEL0
    need0 = mc.sfi_candidates(case["frames"][0][0], case["frames"][1][0], 100)
    later = max(mc.sfi_candidates(follow["frames"][p][0], follow["frames"][p + 1][0], 100) for p in range(3))
    assert need0 > FIRST_POOL and need0 > 1100 and later > FIRST_POOL and later <= need0      # a pool grown for need0 holds the follow-up


@pytest.mark.parametrize("ori", [True, False])
def test_best_only_reference_is_not_vacuous(rag, ori):
    """mode 2's restatement: matches, newly taken keypoints, and with the histogram on some accepted matches removed or none lost"""
    qs = mc.projection_queries(rag, SEED + 1, 200)
    k, d = rag["frames"][5]
    m = qs["nq"][5]
    tk = qs["taken"][5, :len(k)]
    r = mc.best_only_reference(k, d, qs["q"][5, :m], qs["qdesc"][5, :m], qs["qobs"][5, :m], qs["qang"][5, :m], tk, ori)
    accepted = int((r["match"] >= 0).sum())
    assert accepted > 50 and r["nmatches"] <= accepted and (r["nmatches"] == accepted or ori)
    assert r["taken"].sum() > tk.sum() and np.all(r["taken"][tk == 1] == 1)
    assert np.all(tk[r["match"][r["match"] >= 0]] == 0)                 # a taken keypoint is never matched
    unobserved = (r["match"] >= 0) & (qs["qobs"][5, :m] == 0)
    assert unobserved.any()                                           # and an unobserved point's keypoint is not marked by it alone


@pytest.mark.parametrize("chi2", [5.99, 0.0])
def test_fuse_case_has_matches(rag, chi2):
    fc = mc.fuse_case(rag, SEED + 2)
    sf, _, isg, logsf = mc.scale_tables()
    assert fc["nmp"] == 257
    for k in range(8):
        kk, dd = rag["frames"][k]
        bi, bd = oracle.fuse_search(kk, dd, mc.COLS, mc.ROWS, fc["x3"], fc["valid"][k], fc["min_d"], fc["max_d"], fc["nrm"], fc["mp_desc"],
                                    fc["Tcw"][k].reshape(3, 4), fc["Ow"][k], mc.TUM1_K, sf, isg, logsf, 3.0, chi2)
        if _big(rag, k):
            assert (bd <= 50).sum() > 0, k
        if len(kk) == 0:
            assert np.all(bi == -1) and np.all(bd == 256)


@pytest.mark.parametrize("levelsup", [1, 4])
def test_bow_pairs_have_matches(rag, levelsup):
    voc, ovoc = mc.vocabulary(SEED + 3)
    assert (voc["weight"][voc["is_leaf"] == 1] == 0).any()          # stop words exist in this vocabulary
    tr = [ovoc.transform(d, levelsup) for _, d in rag["frames"]]
    assert len(tr[0]["bow"][0]) == 0 and len(tr[0]["fv"][0]) == 0
    assert any((t["weight"] == 0).any() for t in tr)                # and features land on them
    sf, sg, _, _ = mc.scale_tables()
    F12, epi = mc.triangulation_geometry(len(mc.BOW_PAIRS))
    for p, (a, b) in enumerate(mc.BOW_PAIRS + [(f, f + 1) for f in range(7)]):
        (ka, da), (kb, db) = rag["frames"][a], rag["frames"][b]
        for kfkf in (False, True):
            v = (np.arange(384) % 7 != 0).astype(np.uint8)
            n, _, _ = oracle.search_by_bow(ka, da, tr[a]["fv"], kb, db, tr[b]["fv"], v[:len(ka)], v[:len(kb)] if kfkf else None, 0.7, True,
                                           49 if kfkf else 50, 1.0 / 30 if kfkf else 30 / 360.0)
            if _big(rag, a) and _big(rag, b):
                assert n > 0, (a, b, kfkf)
        if p < len(mc.BOW_PAIRS):
            n, _ = oracle.search_for_triangulation(ka, da, tr[a]["fv"], kb, db, tr[b]["fv"], F12[p].reshape(3, 3), epi[p], sf, sg)
            if p == 2:
                assert n == 0                                        # the all-zero F12
            elif _big(rag, a) and _big(rag, b):
                assert n > 0, (a, b)


def test_distinctive_case():
    desc, off = mc.distinctive_case(11, mc.DISTINCTIVE_SIZES + [300])
    want = oracle.distinctive_descriptors(desc[:off[-2]], off[:-1])
    assert (want[1:] >= 0).all() and want[0] == -1
    first256 = oracle.distinctive_descriptors(desc[off[-2]:off[-2] + 256], np.array([0, 256], np.int32))
    assert 0 <= first256[0] < 256
