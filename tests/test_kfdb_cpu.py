"""CPU tests of the KeyFrameDatabase candidate queries: the ABI declares and exports them, the shim compiles and links against the mock
headers, the CPU restatement (tests/kfdb_ref.cpp) equals the reference's recorded outputs (tests/golden/kfdb_cases.npz) bit for bit on
every case, the fixture covers the branches that make such parity mean something, and two second opinions (numpy for the score, an
inverted file in Python for the sharing order) agree with the restatement."""
import os

import numpy as np
import pytest

import kfdb_build as B
import kfdb_cases as S
from test_abi_cpu import _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["orbfe_detect_candidates", "orbfe_detect_candidates_batch_device", "orbfe_bow_min_score_batch_device", "orbfe_bow_score",
       "orbfe_bow_score_batch_device"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "kfdb_cases.npz"))


@pytest.fixture(scope="module")
def ref():
    """the restatement on every case, once"""
    return {n: B.detect(S.case(n)) for n in S.CASES}


def test_header_binding_and_library_agree_on_the_database_queries():
    from orb_slam2_aruco_amd import binding, header
    assert set(NEW) <= set(header.functions), sorted(set(NEW) - set(header.functions))
    assert set(NEW) <= set(binding.SYMBOLS)
    assert set(NEW) <= _exports(), sorted(set(NEW) - _exports())
    rec = header.dtype("orbfe_kfdb_result")
    assert rec == binding.KFDB_RESULT_DTYPE == B.RESULT_DTYPE and rec.itemsize == 36
    for name in ("KFDB_LOOP", "KFDB_RELOC", "KFDB_NEIGHBOURS", "KFDB_MAX_KEYFRAMES", "KFDB_MAX_WORDS"):
        assert header.defines[name] == getattr(binding, name), name
    assert (binding.KFDB_LOOP, binding.KFDB_RELOC, binding.KFDB_MAX_WORDS) == (S.LOOP, S.RELOC, S.CAPACITY) == (B.LOOP, B.RELOC, 4096)
    assert binding.KFDB_MAX_KEYFRAMES >= 4096


def test_fixture_holds_every_case_and_its_inputs_have_not_drifted(golden):
    assert sorted(set(k.split("/")[0] for k in golden.files if "/" in k)) == S.CASES
    for n in S.CASES:
        assert np.array_equal(golden[n + "/digest"], S.digest(S.case(n))), n + ": the case builder no longer gives the recorded inputs"


@pytest.mark.parametrize("name", S.CASES)
def test_restatement_equals_the_reference_bit_for_bit(name, golden, ref):
    r = ref[name]
    assert np.array_equal(r["candidates"], golden[name + "/candidates"])
    assert r["result"].tobytes() == golden[name + "/record"][0].tobytes(), (r["result"], golden[name + "/record"][0])
    assert np.array_equal(r["scores"].view(np.uint32), golden[name + "/scores"])
    assert np.array_equal(r["common"], golden[name + "/common"])
    assert np.array_equal(r["extra"], golden[name + "/extra"])


def test_fixture_covers_the_branches(golden):
    rec = {n: golden[n + "/record"][0] for n in S.CASES}
    extra = {n: golden[n + "/extra"] for n in S.CASES}
    mode = {n: S.case(n)["mode"] for n in S.CASES}
    for m in (S.LOOP, S.RELOC):
        assert sum(mode[n] == m and rec[n]["n_candidates"] >= 2 for n in S.CASES) >= 6, m
    assert sum(rec[n]["n_candidates"] < extra[n][B.N_RETAINED] for n in S.CASES) >= 3          # a duplicate went
    assert sum(extra[n][B.N_BEST_OTHER] > 0 for n in S.CASES) >= 3                            # pBestKF is another keyframe
    assert sum(mode[n] == S.LOOP and rec[n]["n_scored"] > 0 and rec[n]["n_kept"] == 0 for n in S.CASES) >= 2   # empty because of min_score
    assert sum(mode[n] == S.LOOP and extra[n][B.N_KEPT_EQ_MIN] > 0 for n in S.CASES) >= 2     # the >= of the min_score gate
    assert sum(mode[n] == S.RELOC and extra[n][B.N_STALE] > 0 for n in S.CASES) >= 3
    assert {(1, 0), (4, 3), (5, 4)} <= set((int(rec[n]["max_common_words"]), int(rec[n]["min_common_words"])) for n in S.CASES)
    assert sum(len(S.case(n)["q_word"]) > 0 and rec[n]["n_sharing"] == 0 and len(S.case(n)["connected"]) < S.case(n)["K"] for n in S.CASES) >= 1
    assert rec["loop_all_connected"]["n_sharing"] == 0 and len(S.case("loop_all_connected")["connected"]) == S.case("loop_all_connected")["K"]
    sizes = set(S.case(n)["K"] for n in S.CASES)
    assert {1, 2, 63, 64, 65, 300, 600} <= sizes
    counts = set(len(S.case(n)["q_word"]) for n in S.CASES) | set(int(d) for n in S.CASES for d in np.diff(S.case(n)["offsets"]))
    assert {0, 1, 63, 64, 65, 257, S.CAPACITY} <= counts


@pytest.mark.parametrize("name", ["reloc_stale_a", "reloc_stale_b", "reloc_stale_c", "reloc_k64"])
def test_a_stale_score_decides_the_output(name, ref):
    """the neighbours that share a word with the query but were not scored contribute the state the caller passed: with another
    state there the accumulated scores change"""
    c, r = S.case(name), ref[name]
    assert r["extra"][B.N_STALE] > 0
    not_scored = (r["common"] > 0) & (r["common"] <= r["result"]["min_common_words"])
    state = c["scores"].copy()
    state[not_scored] += np.float32(1.0)
    r2 = B.detect(c, scores=state)
    assert r2["result"]["best_acc_score"] != r["result"]["best_acc_score"]
    assert np.array_equal(r2["scores"][~not_scored], r["scores"][~not_scored])       # what the call writes does not depend on it
    state = c["scores"].copy()
    state[r["common"] == 0] += np.float32(1.0)                                       # keyframes that were not met are never read
    r3 = B.detect(c, scores=state)
    assert r3["result"].tobytes() == r["result"].tobytes() and np.array_equal(r3["candidates"], r["candidates"])


@pytest.mark.parametrize("name", ["loop_erased_best", "reloc_erased_best"])
def test_the_erased_keyframe_would_have_been_the_best_candidate(name, ref):
    c = dict(S.case(name))
    gone = int(np.flatnonzero(c["active"] == 0)[0])
    assert gone not in ref[name]["candidates"] and ref[name]["common"][gone] == 0
    c["active"] = np.ones(c["K"], np.uint8)
    r = B.detect(c)
    assert r["scores"][gone] == np.float32(1.0) and gone in r["candidates"] and r["common"][gone] == len(c["q_word"])


@pytest.mark.parametrize("name", ["loop_min_equal_a", "loop_min_equal_b", "loop_min_equal_c"])
def test_a_score_equal_to_min_score_is_kept(name, ref):
    c, r = S.case(name), ref[name]
    assert r["extra"][B.N_KEPT_EQ_MIN] >= 1
    above = B.detect(c, min_score=np.nextafter(c["min_score"], np.float32(2)))
    assert above["result"]["n_kept"] == r["result"]["n_kept"] - r["extra"][B.N_KEPT_EQ_MIN]


def test_score_against_numpy():
    """1 - 0.5 * ||v - w||_1 on the dense vectors: another formula, so agreement to rounding, not bit for bit"""
    rng = np.random.default_rng(5)
    for name in ("reloc_k64", "loop_dense", "reloc_max4", "reloc_capacity"):
        c = S.case(name)
        top = int(max(c["word"].max(), c["q_word"].max())) + 1
        q = np.zeros(top); q[c["q_word"]] = c["q_value"]
        for k in rng.choice(c["K"], min(c["K"], 8), replace=False):
            w, v = c["word"][c["offsets"][k]:c["offsets"][k + 1]], c["value"][c["offsets"][k]:c["offsets"][k + 1]]
            d = np.zeros(top); d[w] = v
            want = 1.0 - 0.5 * np.abs(q - d).sum()
            got = B.score(c["q_word"], c["q_value"], w, v)
            assert abs(got - want) <= 1e-13, (name, k, got, want)
            assert np.float32(got) == S.float_scores((c["q_word"], c["q_value"]), [(w, v)])[0]


def test_score_of_vectors_without_a_common_word_is_minus_zero():
    s = B.score([1, 2], [0.5, 0.5], [3], [1.0])
    assert s == 0.0 and np.signbit(s)


@pytest.mark.parametrize("name", S.CASES)
def test_sharing_order_against_a_brute_force_inverted_file(name, ref):
    order, count = S.brute_force_sharing(S.case(name))
    assert list(ref[name]["order"]) == order
    assert np.array_equal(ref[name]["common"], count)


def test_min_score_is_the_least_score_over_the_connected_keyframes():
    for name in ("loop_k300", "loop_dense", "loop_erased_best"):
        c = S.case(name)
        ok = [p for p in c["connected"] if c["active"] is None or c["active"][p]]
        bows = [(c["word"][c["offsets"][k]:c["offsets"][k + 1]], c["value"][c["offsets"][k]:c["offsets"][k + 1]]) for k in ok]
        want = min([np.float32(1.0)] + list(S.float_scores((c["q_word"], c["q_value"]), bows)))
        assert B.min_score(c) == want
