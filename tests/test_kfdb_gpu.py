"""GPU: orbfe_detect_candidates / orbfe_detect_candidates_batch_device / orbfe_bow_min_score_batch_device / orbfe_bow_score* against
the reference's recorded outputs (tests/golden/kfdb_cases.npz) where a case is in the fixture and against the CPU restatement
(tests/kfdb_ref.cpp) where not.  Every comparison is bit for bit: candidates, counts, records, and scores as uint32."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kfdb_build as B
import kfdb_cases as S
import voc_cases
from pose_opt_device import Dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "kfdb_cases.npz"))


def _host(orbfe, c, scores=None):
    sc = np.array(c["scores"] if scores is None else scores, np.float32)
    cand, common, rec = orbfe.detect_candidates(c["mode"], c["q_word"], c["q_value"], c["offsets"], c["word"], c["value"], c["neigh"], sc,
                                                active=c["active"], connected=c["connected"], min_score=c["min_score"])
    return dict(candidates=cand, common=common, result=rec, scores=sc)


def _same(got, want):
    assert np.array_equal(got["candidates"], want["candidates"]), (got["candidates"], want["candidates"])
    assert got["result"].tobytes() == want["result"].tobytes(), (got["result"], want["result"])
    assert np.array_equal(got["scores"].view(np.uint32), want["scores"].view(np.uint32))
    assert np.array_equal(got["common"], want["common"])


@pytest.mark.parametrize("name", S.CASES)
def test_host_call_equals_the_reference(orbfe, golden, name):
    got = _host(orbfe, S.case(name))
    _same(got, dict(candidates=golden[name + "/candidates"], result=golden[name + "/record"][0], scores=golden[name + "/scores"],
                    common=golden[name + "/common"]))


@pytest.mark.parametrize("mode", [S.LOOP, S.RELOC])
def test_host_call_at_the_largest_database(orbfe, mode):
    """K = 8192 keyframes that all share words with the query: the full sort, the largest LDS block, thousands of kept entries"""
    c = S.traj(mode, 77, orbfe.KFDB_MAX_KEYFRAMES, 12, 40, win=64, slide=0, nneigh=(0, 10), reach=40, erased=0.02, conn=5, min_score=0.01)
    want = B.detect(c)
    assert want["result"]["n_sharing"] > 8000 and want["result"]["n_kept"] > 500 and want["result"]["n_candidates"] >= 1
    _same(_host(orbfe, c), want)


def test_host_call_twice_on_one_state_is_the_sequential_reference(orbfe):
    """a relocalization query leaves its scores behind for the next one"""
    a, b = S.case("reloc_stale_a"), S.traj(S.RELOC, 10, 80, 90, 90, reach=8, nneigh=(6, 10), p_absent=0.05, q0=43)
    assert np.array_equal(a["word"], b["word"]) and not np.array_equal(a["q_word"], b["q_word"])
    w1 = B.detect(a)
    w2 = B.detect(b, scores=w1["scores"])
    assert B.detect(b)["result"].tobytes() != w2["result"].tobytes()      # the first query's state matters to the second
    g1 = _host(orbfe, a)
    _same(g1, w1)
    _same(_host(orbfe, b, scores=g1["scores"]), w2)


# ------------------------------------------------------------------------------------------------ the batch call --
CAP, NF, KDB = 96, 56, 48


@functools.lru_cache(maxsize=None)
def _blocks():
    """NF frames of a synthetic trajectory through orbfe_vocabulary_transform_batch_device: frame f's descriptors come from a window
    of the vocabulary's leaves that slides with f.  Then three blocks are doctored to exercise the count clamp: a count above the
    block over a block filled to its end with ascending words, a negative count, and an empty frame.  Returns the device arrays and
    the BowVectors as the kernels must read them."""
    from orb_slam2_aruco_amd import binding
    voc = voc_cases.make(10, 3, 17, irregular=False)
    gvoc = binding.ORBVocabulary.from_arrays(10, 3, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    rng = np.random.default_rng(99)
    leaves = np.flatnonzero(voc["is_leaf"])
    desc = np.zeros((NF, CAP, 32), np.uint8)
    n = rng.integers(CAP // 2, CAP + 1, NF).astype(np.int32)
    n[5] = 0
    for f in range(NF):
        at = (f % KDB) * 12 if f < KDB else int(rng.integers(0, KDB)) * 12       # the queries sit somewhere along the trajectory
        pick = rng.choice(leaves[at:at + 160], n[f])
        bits = np.unpackbits(voc["desc"][pick], axis=1)
        for i in range(n[f]):
            bits[i, rng.choice(256, 6, replace=False)] ^= 1
        desc[f, :n[f]] = np.packbits(bits, axis=1)
    d = dict(desc=Dev(desc), n=Dev(n), word=Dev(np.zeros((NF, CAP), np.int32)), node=Dev(np.zeros((NF, CAP), np.int32)),
             weight=Dev(np.zeros((NF, CAP))), bw=Dev(np.zeros((NF, CAP), np.uint32)), bv=Dev(np.zeros((NF, CAP))),
             nb=Dev(np.zeros(NF, np.int32)), fn=Dev(np.zeros((NF, CAP), np.uint32)), fo=Dev(np.zeros((NF, CAP + 1), np.int32)),
             ff=Dev(np.zeros((NF, CAP), np.uint32)), nf=Dev(np.zeros(NF, np.int32)))
    rc = gvoc.L.orbfe_vocabulary_transform_batch_device(gvoc.h, d["desc"].ptr, d["n"].ptr, CAP, NF, 2, d["word"].ptr, d["node"].ptr,
                                                        d["weight"].ptr, d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, d["fn"].ptr, d["fo"].ptr,
                                                        d["ff"].ptr, d["nf"].ptr, None)
    assert rc == 0, gvoc.L.orbfe_last_error()
    bw, bv, nb = d["bw"].get(), d["bv"].get(), d["nb"].get()
    assert nb[5] == 0 and nb.max() <= CAP and nb[7] > 8
    # frame 7: its block filled to the end, its count beyond the block; frame 9: a negative count
    bw[7, nb[7]:] = bw[7, nb[7] - 1] + 1 + np.arange(CAP - nb[7], dtype=np.uint32) * 3
    bv[7, nb[7]:] = 0.001
    nb[7], nb[9] = CAP + 9, -4
    d["bw"].put(bw); d["bv"].put(bv); d["nb"].put(nb)
    bows = [(bw[f, :min(max(nb[f], 0), CAP)].copy(), bv[f, :min(max(nb[f], 0), CAP)].copy()) for f in range(NF)]
    assert all(np.all(np.diff(w.astype(np.int64)) > 0) for w, _ in bows)
    return d, bows


def _batch_case(mode, db, queries, seed):
    """the restatement's view of a batch: one case per query over the database `db` (frame indices in add order)"""
    _, bows = _blocks()
    rng = np.random.default_rng(seed)
    K = len(db)
    active = (rng.random(K) >= 0.08).astype(np.uint8)
    neigh = np.full((K, 10), -1, np.int32)
    for k in range(K):
        near = [p for p in range(k - 6, k + 7) if p != k and 0 <= p < K]
        row = [int(p) if rng.random() >= 0.15 else -2 for p in rng.permutation(near)[:int(rng.integers(0, 11))]]
        neigh[k, :len(row)] = row
    conn = [np.sort(rng.choice(K, int(rng.integers(0, 6)), replace=False)).astype(np.int32) for _ in queries]
    min_score = (rng.random(len(queries)) * 0.05).astype(np.float32)
    state = (rng.random((len(queries), K)) * 0.4).astype(np.float32)
    cases = [S._finish(mode, bows[q], [bows[f] for f in db], active, neigh, conn[i] if mode == S.LOOP else [], min_score[i], state[i])
             for i, q in enumerate(queries)]
    return cases, active, neigh, conn, min_score, state


def _run_batch(orbfe, mode, db, d_db, queries, active, neigh, conn, min_score, state, d_min_score=None):
    d, _ = _blocks()
    K, nq = len(db), len(queries)
    off = np.zeros(nq + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in conn])
    d_q, d_act, d_ng = Dev(np.array(queries, np.int32)), Dev(active), Dev(neigh)
    d_co, d_c = Dev(off), Dev(np.concatenate(conn + [np.zeros(0, np.int32)]).astype(np.int32))
    d_ms = d_min_score or Dev(min_score)
    d_sc, d_cand = Dev(state), Dev(np.full((nq, K), -77, np.int32))
    d_com, d_scr, d_res = Dev(np.full((nq, K), -5, np.int32)), Dev(np.zeros((nq, K), np.uint32)), Dev(np.zeros(nq, orbfe.KFDB_RESULT_DTYPE))
    orbfe.detect_candidates_batch_device(mode, d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, CAP, None if d_db is None else d_db.ptr, d_act.ptr, K,
                                         d_q.ptr, nq, d_ng.ptr, d_co.ptr, d_c.ptr, d_ms.ptr, d_sc.ptr, d_cand.ptr, d_com.ptr, d_scr.ptr,
                                         d_res.ptr, None)
    return d_sc.get(), d_cand.get(), d_com.get(), d_res.get()


@pytest.mark.parametrize("mode", [S.LOOP, S.RELOC])
@pytest.mark.parametrize("nq,permuted", [(1, False), (3, True), (8, False), (8, True)])
def test_batch_call_equals_the_restatement(orbfe, mode, nq, permuted):
    rng = np.random.default_rng(nq * 2 + permuted)
    db = list(rng.permutation(KDB)) if permuted else list(range(KDB))
    queries = [KDB + i for i in range(nq - 1)] + [int(db[20])]          # the last query is in the database
    if nq >= 3:
        queries[1] = 5                                                  # an empty query
    cases, active, neigh, conn, min_score, state = _batch_case(mode, db, queries, 300 + nq)
    sc, cand, com, res = _run_batch(orbfe, mode, db, Dev(np.array(db, np.int32)) if permuted else None, queries, active, neigh, conn,
                                    min_score, state)
    ncand = 0
    for i, c in enumerate(cases):
        want = B.detect(c)
        nc = int(res[i]["n_candidates"])
        _same(dict(candidates=cand[i, :nc], common=com[i], result=res[i], scores=sc[i]), want)
        assert np.all(cand[i, nc:] == -77)                              # the rest of the row is the caller's
        ncand += nc
    assert ncand >= 1                                                    # the batch is not a row of empty answers
    c_in = cases[-1]                                                     # the query that is in the database finds itself
    k_self = db.index(queries[-1])
    if active[k_self] and queries[-1] not in (5, 7, 9) and not (mode == S.LOOP and k_self in conn[-1]):
        assert com[-1, k_self] == len(c_in["q_word"]) and sc[-1, k_self] == np.float32(1.0)


def test_batch_two_queries_on_one_state_row_are_sequential(orbfe):
    db = list(range(KDB))
    cases, active, neigh, conn, min_score, state = _batch_case(S.RELOC, db, [KDB, KDB + 1], 410)
    w1 = B.detect(cases[0])
    w2 = B.detect(cases[1], scores=w1["scores"])
    d, _ = _blocks()
    d_act, d_ng, d_sc = Dev(active), Dev(neigh), Dev(state[0])
    outs = []
    for q in (KDB, KDB + 1):                                             # two launches on the null stream, one row of state
        d_q, d_cand, d_com = Dev(np.array([q], np.int32)), Dev(np.full(KDB, -77, np.int32)), Dev(np.zeros(KDB, np.int32))
        d_scr, d_res = Dev(np.zeros(KDB, np.uint32)), Dev(np.zeros(1, orbfe.KFDB_RESULT_DTYPE))
        orbfe.detect_candidates_batch_device(S.RELOC, d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, CAP, None, d_act.ptr, KDB, d_q.ptr, 1, d_ng.ptr,
                                             None, None, None, d_sc.ptr, d_cand.ptr, d_com.ptr, d_scr.ptr, d_res.ptr, None)
        outs.append((d_cand, d_com, d_res))
    for (d_cand, d_com, d_res), want in zip(outs, (w1, w2)):
        res = d_res.get()[0]
        assert res.tobytes() == want["result"].tobytes()
        assert np.array_equal(d_cand.get()[:res["n_candidates"]], want["candidates"]) and np.array_equal(d_com.get(), want["common"])
    assert np.array_equal(d_sc.get().view(np.uint32), w2["scores"].view(np.uint32))


def test_chain_min_score_then_candidates_on_one_stream(orbfe):
    """DetectLoop's head: orbfe_bow_min_score_batch_device writes d_min_score, orbfe_detect_candidates_batch_device reads it on the
    device; nothing is downloaded in between"""
    db = list(range(KDB))
    queries = [KDB + i for i in range(6)]
    cases, active, neigh, conn, _, state = _batch_case(S.LOOP, db, queries, 520)
    conn[2] = np.zeros(0, np.int32)                                       # no connected keyframe: minScore stays 1
    cases[2]["connected"] = conn[2]
    d, _ = _blocks()
    off = np.zeros(len(queries) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in conn])
    d_ms = Dev(np.full(len(queries), -3, np.float32))
    d_q, d_act, d_co = Dev(np.array(queries, np.int32)), Dev(active), Dev(off)
    d_c = Dev(np.concatenate(conn + [np.zeros(0, np.int32)]).astype(np.int32))
    orbfe.bow_min_score_batch_device(d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, CAP, None, d_act.ptr, KDB, d_q.ptr, len(queries), d_co.ptr, d_c.ptr,
                                     d_ms.ptr, None)
    sc, cand, com, res = _run_batch(orbfe, S.LOOP, db, None, queries, active, neigh, conn, None, state, d_min_score=d_ms)
    ms = d_ms.get()
    assert ms[2] == np.float32(1.0)
    for i, c in enumerate(cases):
        want_ms = B.min_score(c)
        assert ms[i].tobytes() == want_ms.tobytes(), (i, ms[i], want_ms)
        want = B.detect(c, min_score=want_ms)
        _same(dict(candidates=cand[i, :res[i]["n_candidates"]], common=com[i], result=res[i], scores=sc[i]), want)


def test_raw_scores_host_and_device(orbfe):
    d, bows = _blocks()
    rng = np.random.default_rng(8)
    p1, p2 = rng.integers(0, NF, 40).astype(np.int32), rng.integers(0, NF, 40).astype(np.int32)
    p1[:4], p2[:4] = [5, 10, 9, 7], [6, 10, 7, 8]                        # the empty, a frame with itself, the negative-count and the over-full frame
    want = np.array([np.float32(B.score(bows[a][0], bows[a][1], bows[b][0], bows[b][1])) for a, b in zip(p1, p2)], np.float32)
    d_out, d_p1, d_p2 = Dev(np.full(40, -3, np.float32)), Dev(p1), Dev(p2)
    orbfe.bow_score_batch_device(d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, CAP, d_p1.ptr, d_p2.ptr, 40, d_out.ptr, None)
    assert np.array_equal(d_out.get().view(np.uint32), want.view(np.uint32))
    off, word, value = S._csr(bows)
    assert np.array_equal(orbfe.bow_score(off, word, value, p1, p2).view(np.uint32), want.view(np.uint32))
    assert want[1] == np.float32(1.0) and np.signbit(want[0]) and want[0] == 0


# ------------------------------------------------------------------------------------------- errors and capacity --
def _raw_host(orbfe, c, **over):
    """orbfe_detect_candidates itself with canaries in every output -> (rc, whether nothing was written)"""
    a = dict(mode=c["mode"], scoring=0, q_word=c["q_word"], q_value=c["q_value"], nbow=len(c["q_word"]), offsets=c["offsets"], word=c["word"],
             value=c["value"], active=c["active"], K=c["K"], neigh=c["neigh"], connected=c["connected"], nconn=len(c["connected"]),
             min_score=float(c["min_score"]))
    a.update(over)
    K = c["K"]
    scores, cand, common = c["scores"].copy(), np.full(K, -77, np.int32), np.full(K, -77, np.int32)
    res = np.full(1, -77, np.int32).repeat(9).view(orbfe.KFDB_RESULT_DTYPE)
    p = lambda x: None if x is None else np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(a[k]) if a[k] is not None else None for k in ("q_word", "q_value", "offsets", "word", "value", "active", "neigh", "connected")]
    rc = orbfe.load().orbfe_detect_candidates(a["mode"], a["scoring"], p(keep[0]), p(keep[1]), a["nbow"], p(keep[2]), p(keep[3]), p(keep[4]),
                                              p(keep[5]), a["K"], p(keep[6]), p(keep[7]), a["nconn"], a["min_score"], p(scores), p(cand),
                                              p(common), p(res), 0)
    untouched = np.array_equal(scores.view(np.uint32), c["scores"].view(np.uint32)) and np.all(cand == -77) and np.all(common == -77) and \
        np.all(res.view(np.int32) == -77)
    return rc, untouched


def test_host_call_errors_write_nothing(orbfe):
    c = S.case("loop_k63")
    assert _raw_host(orbfe, c)[0] == orbfe.ORBFE_OK
    swapped = c["q_word"].copy(); swapped[[3, 4]] = swapped[[4, 3]]
    db_swapped = c["word"].copy(); db_swapped[[0, 1]] = db_swapped[[1, 0]]
    dup = c["q_word"].copy(); dup[1] = dup[0]
    off1 = c["offsets"].copy(); off1[0] = 1
    offd = c["offsets"].copy(); offd[5] = offd[4] - 1
    nan_q = c["q_value"].copy(); nan_q[2] = np.nan
    inf_v = c["value"].copy(); inf_v[-1] = np.inf
    big_ng = c["neigh"].copy(); big_ng[3, 9] = c["K"]
    bad = dict(mode=dict(mode=2), scoring=dict(scoring=1), q_order=dict(q_word=swapped), q_dup=dict(q_word=dup),
               db_order=dict(word=db_swapped), off_start=dict(offsets=off1), off_decreasing=dict(offsets=offd), nan=dict(q_value=nan_q),
               inf=dict(value=inf_v), neigh=dict(neigh=big_ng), conn_high=dict(connected=np.array([c["K"]], np.int32), nconn=1),
               conn_neg=dict(connected=np.array([-1], np.int32), nconn=1), min_score=dict(min_score=float("nan")),
               null_query=dict(q_word=None), null_offsets=dict(offsets=None), null_neigh=dict(neigh=None), negative_nbow=dict(nbow=-1))
    for what, over in bad.items():
        rc, untouched = _raw_host(orbfe, c, **over)
        assert rc == orbfe.ORBFE_ERR_INVALID and untouched, what
    # above the bounds of the batch call
    wide = S.tiny(S.RELOC, range(orbfe.KFDB_MAX_WORDS + 1), [[1, 2]])
    rc, untouched = _raw_host(orbfe, wide)
    assert rc == orbfe.ORBFE_ERR_CAPACITY and untouched
    many = S.tiny(S.RELOC, [1], [[1]] * (orbfe.KFDB_MAX_KEYFRAMES + 1))
    rc, untouched = _raw_host(orbfe, many)
    assert rc == orbfe.ORBFE_ERR_CAPACITY and untouched


def test_batch_call_errors_and_skipped_queries(orbfe):
    L = orbfe.load()
    d, _ = _blocks()
    db = list(range(KDB))
    queries = [KDB, KDB + 1, KDB + 2]
    cases, active, neigh, conn, min_score, state = _batch_case(S.LOOP, db, queries, 630)
    nq = 3
    bufs = dict(q=Dev(np.array(queries, np.int32)), act=Dev(active), ng=Dev(neigh), co=Dev(np.zeros(nq + 1, np.int32)), c=Dev(np.zeros(8, np.int32)),
                ms=Dev(min_score), sc=Dev(state), cand=Dev(np.full((nq, KDB), -77, np.int32)), com=Dev(np.full((nq, KDB), -77, np.int32)),
                scr=Dev(np.zeros((nq, KDB), np.uint32)), res=Dev(np.full(nq * 9, -77, np.int32)))

    def call(mode=S.LOOP, scoring=0, cap=CAP, K=KDB, n=nq, **null):
        g = lambda k: None if k in null else bufs[k].ptr
        return L.orbfe_detect_candidates_batch_device(mode, scoring, d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, cap, None, g("act"), K, g("q"), n, g("ng"),
                                                      g("co"), g("c"), g("ms"), g("sc"), g("cand"), g("com"), g("scr"), g("res"), None)
    assert call(mode=3) == orbfe.ORBFE_ERR_INVALID and call(scoring=2) == orbfe.ORBFE_ERR_INVALID
    assert call(K=0) == orbfe.ORBFE_ERR_INVALID and call(n=-1) == orbfe.ORBFE_ERR_INVALID and call(cap=0) == orbfe.ORBFE_ERR_INVALID
    for k in ("q", "ng", "co", "c", "ms", "sc", "cand", "com", "scr", "res"):
        assert call(**{k: True}) == orbfe.ORBFE_ERR_INVALID, k
    assert call(K=orbfe.KFDB_MAX_KEYFRAMES + 1) == orbfe.ORBFE_ERR_CAPACITY
    assert call(cap=orbfe.KFDB_MAX_WORDS + 1) == orbfe.ORBFE_ERR_CAPACITY and call(n=65536) == orbfe.ORBFE_ERR_CAPACITY
    assert L.orbfe_bow_min_score_batch_device(0, d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, orbfe.KFDB_MAX_WORDS + 1, None, None, KDB, bufs["q"].ptr, nq,
                                              bufs["co"].ptr, bufs["c"].ptr, bufs["ms"].ptr, None) == orbfe.ORBFE_ERR_CAPACITY
    assert L.orbfe_bow_score_batch_device(1, d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, CAP, bufs["q"].ptr, bufs["q"].ptr, nq, bufs["ms"].ptr, None) == orbfe.ORBFE_ERR_INVALID
    assert call(n=0) == orbfe.ORBFE_OK
    for k in ("sc", "cand", "com", "res"):                                # none of the calls above wrote anything
        assert np.array_equal(bufs[k].get(), bufs[k].a), k
    # a query with a connected position outside the database, and one whose range decreases, are skipped; the third runs
    bufs["co"].put(np.array([0, 2, 1, 5], np.int32))                     # query 1: [2, 1) decreases; query 2: [1, 5)
    bufs["c"].put(np.array([3, KDB, 4, 5, 6, 0, 0, 0], np.int32))
    assert call() == orbfe.ORBFE_OK
    res = bufs["res"].get().view(orbfe.KFDB_RESULT_DTYPE)
    cand, com, sc = bufs["cand"].get(), bufs["com"].get(), bufs["sc"].get()
    for i in (0, 1):
        assert res[i]["status"] == orbfe.ORBFE_ERR_INVALID and all(res[i][f] == 0 for f in res.dtype.names if f != "status")
        assert np.all(cand[i] == -77) and np.all(com[i] == 0) and np.array_equal(sc[i].view(np.uint32), state[i].view(np.uint32))
    assert res[2]["status"] == orbfe.ORBFE_ERR_INVALID                    # its range [1, 5) holds the position KDB too
    bufs["co"].put(np.array([0, 0, 0, 3], np.int32))
    bufs["c"].put(np.array([4, 5, 6, 0, 0, 0, 0, 0], np.int32))
    assert call() == orbfe.ORBFE_OK
    res = bufs["res"].get().view(orbfe.KFDB_RESULT_DTYPE)
    c2 = dict(cases[2], connected=np.array([4, 5, 6], np.int32))
    want = B.detect(c2)
    assert res[2].tobytes() == want["result"].tobytes() and res[2]["status"] == orbfe.ORBFE_OK
    assert np.array_equal(bufs["cand"].get()[2, :res[2]["n_candidates"]], want["candidates"])


def test_raw_score_and_min_score_calls_errors_write_nothing(orbfe):
    """every ORBFE_ERR_INVALID / ORBFE_ERR_CAPACITY condition of orbfe_bow_score, orbfe_bow_score_batch_device and
    orbfe_bow_min_score_batch_device, each with canaries in the output"""
    L = orbfe.load()
    INV, CAPY = orbfe.ORBFE_ERR_INVALID, orbfe.ORBFE_ERR_CAPACITY
    d, bows = _blocks()
    off, word, value = S._csr(bows[:12])
    p1, p2 = np.array([0, 3, 11, 4], np.int32), np.array([1, 3, 2, 10], np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

    def host(scoring=0, nframes=12, npairs=4, **over):
        a = dict(off=off, word=word, value=value, p1=p1, p2=p2)
        a.update(over)
        keep = {k: None if v is None else np.ascontiguousarray(v) for k, v in a.items()}
        out = np.full(4, -77, np.float32)
        rc = L.orbfe_bow_score(scoring, p(keep["off"]), p(keep["word"]), p(keep["value"]), nframes, p(keep["p1"]), p(keep["p2"]), npairs, p(out), 0)
        return rc, bool(np.all(out == -77))
    rc, untouched = host()
    assert rc == orbfe.ORBFE_OK and not untouched
    first = int(off[3])                                                   # frame 3 has words: frames 5, 7, 9 of the set are the odd ones
    unsorted = word.copy(); unsorted[[first, first + 1]] = unsorted[[first + 1, first]]
    twice = word.copy(); twice[first + 1] = twice[first]
    off1 = off.copy(); off1[0] = 1
    offd = off.copy(); offd[4] = offd[3] - 1
    nan = value.copy(); nan[first] = np.nan
    inf = value.copy(); inf[-1] = -np.inf
    bad = dict(scoring=dict(scoring=1), scoring_dot=dict(scoring=5), pair_negative=dict(p1=np.array([0, -1, 11, 4], np.int32)),
               pair_high=dict(p2=np.array([1, 3, 12, 10], np.int32)), words_unsorted=dict(word=unsorted), word_twice=dict(word=twice),
               offsets_start=dict(off=off1), offsets_decrease=dict(off=offd), nan=dict(value=nan), inf=dict(value=inf), null_offsets=dict(off=None),
               null_word=dict(word=None), null_value=dict(value=None), null_pair1=dict(p1=None), null_pair2=dict(p2=None),
               negative_frames=dict(nframes=-1), negative_pairs=dict(npairs=-1))
    for what, over in bad.items():
        assert host(**over) == (INV, True), what
    assert L.orbfe_bow_score(0, p(off), p(word), p(value), 12, p(p1), p(p2), 4, None, 0) == INV     # no scores array
    assert host(npairs=0) == (orbfe.ORBFE_OK, True)

    # the device calls: what the host can see of their arguments
    bufs = dict(bw=d["bw"], bv=d["bv"], nb=d["nb"], q=Dev(np.array([KDB, KDB + 1], np.int32)), co=Dev(np.array([0, 2, 3], np.int32)),
                c=Dev(np.array([1, 2, 3], np.int32)), ms=Dev(np.full(2, -77, np.float32)), p1=Dev(p1), p2=Dev(p2), sc=Dev(np.full(4, -77, np.float32)))

    def min_score(scoring=0, cap=CAP, K=KDB, n=2, **null):
        g = lambda k: None if k in null else bufs[k].ptr
        return L.orbfe_bow_min_score_batch_device(scoring, g("bw"), g("bv"), g("nb"), cap, None, None, K, g("q"), n, g("co"), g("c"), g("ms"), None)

    def pairs(scoring=0, cap=CAP, n=4, **null):
        g = lambda k: None if k in null else bufs[k].ptr
        return L.orbfe_bow_score_batch_device(scoring, g("bw"), g("bv"), g("nb"), cap, g("p1"), g("p2"), n, g("sc"), None)
    assert min_score(scoring=1) == INV and min_score(cap=0) == INV and min_score(cap=-3) == INV and min_score(K=0) == INV and min_score(K=-1) == INV
    assert min_score(n=-1) == INV and min_score(cap=orbfe.KFDB_MAX_WORDS + 1) == CAPY and min_score(n=0) == orbfe.ORBFE_OK
    for k in ("bw", "bv", "nb", "q", "co", "c", "ms"):
        assert min_score(**{k: True}) == INV, k
    assert pairs(scoring=3) == INV and pairs(cap=0) == INV and pairs(n=-1) == INV and pairs(n=0) == orbfe.ORBFE_OK
    for k in ("bw", "bv", "nb", "p1", "p2", "sc"):
        assert pairs(**{k: True}) == INV, k
    assert np.all(bufs["ms"].get() == -77) and np.all(bufs["sc"].get() == -77)
    assert min_score() == orbfe.ORBFE_OK and pairs() == orbfe.ORBFE_OK        # and the same buffers are written by the good calls
    assert np.all(bufs["ms"].get() != -77) and np.all(bufs["sc"].get() != -77)


def test_chain_candidates_into_search_by_bow_pair_lists(orbfe):
    """orbfe_detect_candidates_batch_device -> orbfe_search_by_bow_batch_device on one stream without reading n_candidates back: each
    row of d_candidates is filled with the query's frame before the call, the next step runs over the first ROWS entries of the row
    as its d_pair2 (d_db = NULL: positions are frames).  Equal to SearchByBoW over the restatement's candidates, padded the same way"""
    L = orbfe.load()
    ROWS = 4
    d, _ = _blocks()
    db, queries = list(range(KDB)), [KDB, KDB + 3]
    cases, active, neigh, conn, min_score, state = _batch_case(S.RELOC, db, queries, 740)
    nq = len(queries)
    d_q, d_act, d_ng, d_sc = Dev(np.array(queries, np.int32)), Dev(active), Dev(neigh), Dev(state)
    d_cand = Dev(np.repeat(np.array(queries, np.int32)[:, None], KDB, axis=1))            # every entry a valid frame: the query itself
    d_com, d_scr, d_res = Dev(np.zeros((nq, KDB), np.int32)), Dev(np.zeros((nq, KDB), np.uint32)), Dev(np.zeros(nq, orbfe.KFDB_RESULT_DTYPE))
    d_kps = Dev(np.zeros((NF, CAP), orbfe.KP_DTYPE))

    def search(d_pair1, pair2_ptr):
        out = Dev(np.full((ROWS, CAP), -9, np.int32)), Dev(np.full((ROWS, CAP), -9, np.int32)), Dev(np.full(ROWS, -9, np.int32))
        rc = L.orbfe_search_by_bow_batch_device(d_kps.ptr, d["desc"].ptr, None, d["n"].ptr, d["fn"].ptr, d["fo"].ptr, d["ff"].ptr, d["nf"].ptr, CAP,
                                                d_pair1.ptr, pair2_ptr, ROWS, 0, 0.75, 0, 50, np.float32(1.0 / 30), out[0].ptr, out[1].ptr,
                                                out[2].ptr, None)
        assert rc == 0, L.orbfe_last_error()
        return out
    orbfe.detect_candidates_batch_device(S.RELOC, d["bw"].ptr, d["bv"].ptr, d["nb"].ptr, CAP, None, d_act.ptr, KDB, d_q.ptr, nq, d_ng.ptr, None,
                                         None, None, d_sc.ptr, d_cand.ptr, d_com.ptr, d_scr.ptr, d_res.ptr, None)
    d_p1 = [Dev(np.full(ROWS, q, np.int32)) for q in queries]
    chained = [search(d_p1[i], d_cand.ptr + i * KDB * 4) for i in range(nq)]              # nothing downloaded up to here
    matched = 0
    for i, (q, c) in enumerate(zip(queries, cases)):
        want = B.detect(c)
        assert 1 <= len(want["candidates"]) <= ROWS
        pair2 = np.full(ROWS, q, np.int32)
        pair2[:len(want["candidates"])] = want["candidates"]
        d_p2 = Dev(pair2)
        direct = search(d_p1[i], d_p2.ptr)
        for got, exp in zip(chained[i], direct):
            assert np.array_equal(got.get(), exp.get())
        nm = chained[i][2].get()
        assert np.all(nm >= 0)
        matched += int(nm[:len(want["candidates"])].sum())
    assert matched > 0
