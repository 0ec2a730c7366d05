"""Seeded inputs of the KeyFrameDatabase query tests (test infrastructure): a "trajectory" of keyframes whose word sets slide over a
word pool, so that neighbours share many words and distant keyframes few; L1-normalised positive values; covisibility tables of 0
to 10 entries with negative (absent) and erased entries; connected sets around the query; a score state that is not zero.

case(name) -> dict: mode, q_word, q_value, K, offsets, word, value (CSR in add order), active (K uint8, or None), neigh (K x 10),
connected, min_score, scores (the state before the call).  CASES lists every name; tests/golden/kfdb_cases.npz holds what the
reference's own code returns for each (tests/gen_kfdb_golden.py) and digest(case) of the inputs it was run on."""
import hashlib

import numpy as np

LOOP, RELOC = 0, 1
CAPACITY = 4096


def _bow(rng, ids, n):
    """n words of ids (sorted), values positive with sum 1"""
    w = np.sort(rng.choice(ids, size=n, replace=False)).astype(np.uint32)
    v = rng.random(n) + 0.05
    return w, v / v.sum() if n else v


def _csr(bows):
    off = np.zeros(len(bows) + 1, np.int32)
    off[1:] = np.cumsum([len(w) for w, _ in bows])
    word = np.concatenate([w for w, _ in bows] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    value = np.concatenate([v for _, v in bows] + [np.zeros(0)]).astype(np.float64)
    return off, word, value


def _finish(mode, q, bows, active, neigh, connected, min_score, scores):
    off, word, value = _csr(bows)
    K = len(bows)
    return dict(mode=mode, q_word=np.ascontiguousarray(q[0], np.uint32), q_value=np.ascontiguousarray(q[1], np.float64), K=K, offsets=off,
                word=word, value=value, active=None if active is None else np.ascontiguousarray(active, np.uint8),
                neigh=np.ascontiguousarray(neigh, np.int32).reshape(K, 10), connected=np.ascontiguousarray(connected, np.int32),
                min_score=np.float32(min_score), scores=np.ascontiguousarray(scores, np.float32))


def float_scores(q, bows):
    """(float)L1 score of the query against every keyframe, by the formula 1 - 0.5 * ||v - w||_1 restricted to the common words, in
    the reference's summation order (numpy scalars are IEEE doubles: the same bits)"""
    out = np.zeros(len(bows), np.float32)
    for k, (w, v) in enumerate(bows):
        _, iq, ik = np.intersect1d(q[0], w, assume_unique=True, return_indices=True)
        s = 0.0
        for a, b in zip(q[1][iq], v[ik]):
            s += abs(a - b) - abs(a) - abs(b)
        out[k] = np.float32(-s / 2.0)
    return out


def traj(mode, seed, K, nk, nq, win=None, slide=None, q0=None, nneigh=(0, 10), reach=6, p_absent=0.15, erased=0.0, conn=3, min_score=0.0,
         min_score_rank=None, state=0.3, query_in_db=False):
    """nk: words per keyframe (an int, or a list cycled over the keyframes); nq: words of the query; win: the pool window a keyframe
    draws from; slide: how far the window moves per keyframe; q0: where on the trajectory the query sits; conn: loop mode, positions
    within conn of q0 are connected; min_score_rank r: min_score = the r-th best float score among the candidates-to-be"""
    rng = np.random.default_rng(seed)
    nks = [nk] if isinstance(nk, int) else list(nk)
    big = max(max(nks), nq, 1)
    win = win or 2 * big
    slide = slide if slide is not None else max(1, win // 8)
    q0 = K // 2 if q0 is None else q0
    pool = np.sort(rng.choice(1 << 20, size=(K + 1) * slide + win, replace=False))
    bows = [_bow(rng, pool[k * slide:k * slide + win], nks[k % len(nks)]) for k in range(K)]
    q = bows[q0] if query_in_db else _bow(rng, pool[q0 * slide:q0 * slide + win], nq)
    active = None
    if erased > 0:
        active = (rng.random(K) >= erased).astype(np.uint8)
    neigh = np.full((K, 10), -1, np.int32)
    for k in range(K):
        n = int(rng.integers(nneigh[0], nneigh[1] + 1))
        near = [p for p in range(k - reach, k + reach + 1) if p != k and 0 <= p < K]
        pick = list(rng.permutation(near)[:n]) if near else []
        row = [int(p) if rng.random() >= p_absent else -1 - int(rng.integers(0, 3)) for p in pick]
        neigh[k, :len(row)] = row
    connected = np.array([p for p in range(q0 - conn, q0 + conn + 1) if 0 <= p < K], np.int32) if mode == LOOP and conn >= 0 else np.zeros(0, np.int32)
    connected = rng.permutation(connected).astype(np.int32)
    if min_score_rank is not None:
        s = float_scores(q, bows)
        ok = np.ones(K, bool) if active is None else active.astype(bool)
        ok[connected] = False
        min_score = np.sort(s[ok])[::-1][min_score_rank]
    scores = (rng.random(K) * state).astype(np.float32)
    return _finish(mode, q, bows, active, neigh, connected, min_score, scores)


def tiny(mode, q_words, kf_words, neigh=None, active=None, connected=(), min_score=0.0, scores=None, seed=0):
    """explicit word sets: values positive with sum 1 per vector, drawn from the seed"""
    rng = np.random.default_rng(1000 + seed)

    def vec(ws):
        v = rng.random(len(ws)) + 0.05
        return np.array(sorted(ws), np.uint32), v / v.sum() if len(ws) else v
    bows = [vec(ws) for ws in kf_words]
    K = len(bows)
    ng = np.full((K, 10), -1, np.int32)
    for k, row in enumerate(neigh or []):
        ng[k, :len(row)] = row
    sc = np.full(K, 0.125, np.float32) if scores is None else scores
    return _finish(mode, vec(q_words), bows, active, ng, connected, min_score, sc)


def erased_best(mode, seed):
    """the keyframe that would have been the best candidate -- the query's own BowVector, score 1 -- has been erased"""
    c = traj(mode, seed, 40, 60, 60, conn=2)
    K, q0 = c["K"], 10   # far from the connected set
    bows = [(c["word"][c["offsets"][k]:c["offsets"][k + 1]], c["value"][c["offsets"][k]:c["offsets"][k + 1]]) for k in range(K)]
    bows[q0] = (c["q_word"].copy(), c["q_value"].copy())
    active = np.ones(K, np.uint8)
    active[q0] = 0
    c["neigh"][q0 + 1, 0] = q0   # and it is somebody's first neighbour
    return _finish(mode, (c["q_word"], c["q_value"]), bows, active, c["neigh"], c["connected"], c["min_score"], c["scores"])


def at_capacity(mode, seed):
    """query and keyframes of CAPACITY words"""
    return traj(mode, seed, 5, [CAPACITY, 3000, CAPACITY], CAPACITY, win=CAPACITY + 600, slide=150, q0=2, nneigh=(2, 4), conn=0)


_B = {
    # sizes: K in {1, 2, 63, 64, 65, 300, 600}, words in {0, 1, 63, 64, 65, 257}
    "reloc_k1": lambda: traj(RELOC, 1, 1, 64, 63),
    "reloc_k2": lambda: traj(RELOC, 2, 2, 65, 64),
    "reloc_k63": lambda: traj(RELOC, 3, 63, [63, 64, 65, 1, 0], 65),
    "reloc_k64": lambda: traj(RELOC, 4, 64, 257, 257),
    "reloc_k65": lambda: traj(RELOC, 5, 65, [64, 257, 65], 63, win=520),
    "reloc_k300": lambda: traj(RELOC, 6, 300, 120, 120, erased=0.1),
    "reloc_k600": lambda: traj(RELOC, 7, 600, [100, 140], 130, erased=0.05, reach=9),
    "reloc_words1": lambda: traj(RELOC, 8, 30, 1, 1, win=4, slide=1),
    "reloc_query0": lambda: traj(RELOC, 9, 20, 64, 0),
    "reloc_stale_a": lambda: traj(RELOC, 10, 80, 90, 90, reach=8, nneigh=(6, 10), p_absent=0.05),
    "reloc_stale_b": lambda: traj(RELOC, 11, 120, 200, 180, reach=10, nneigh=(8, 10), state=0.9),
    "reloc_stale_c": lambda: traj(RELOC, 12, 65, 64, 64, reach=7, nneigh=(5, 10), erased=0.1, state=0.6),
    "reloc_dense": lambda: traj(RELOC, 13, 100, 150, 150, win=200, slide=4),
    "reloc_in_db": lambda: traj(RELOC, 14, 50, 80, 80, query_in_db=True),
    "reloc_erased_best": lambda: erased_best(RELOC, 15),
    "reloc_capacity": lambda: at_capacity(RELOC, 16),
    "loop_k1": lambda: traj(LOOP, 21, 1, 65, 64, conn=-1),
    "loop_k2": lambda: traj(LOOP, 22, 2, 63, 65, conn=-1),
    "loop_k63": lambda: traj(LOOP, 23, 63, [65, 63, 1, 64], 64, conn=2),
    "loop_k64": lambda: traj(LOOP, 24, 64, 257, 257, conn=1, min_score=0.05),
    "loop_k65": lambda: traj(LOOP, 25, 65, [257, 64], 65, win=520, conn=2),
    "loop_k300": lambda: traj(LOOP, 26, 300, 120, 120, erased=0.1, conn=5, min_score=0.02),
    "loop_k600": lambda: traj(LOOP, 27, 600, [100, 140], 130, erased=0.05, reach=9, conn=3, min_score=0.03),
    "loop_dense": lambda: traj(LOOP, 28, 100, 150, 150, win=200, slide=4, conn=2, min_score=0.1),
    "loop_wide": lambda: traj(LOOP, 29, 90, 90, 90, reach=8, nneigh=(6, 10), conn=1, min_score=0.01),
    "loop_loose": lambda: traj(LOOP, 30, 150, 200, 200, win=260, slide=6, conn=3, min_score=0.0),
    "loop_min_too_high_a": lambda: traj(LOOP, 31, 80, 100, 100, conn=2, min_score=0.99),
    "loop_min_too_high_b": lambda: traj(LOOP, 32, 64, 64, 64, conn=1, min_score=0.75),
    "loop_min_equal_a": lambda: traj(LOOP, 33, 80, 100, 100, conn=2, min_score_rank=0),
    "loop_min_equal_b": lambda: traj(LOOP, 34, 65, 65, 65, conn=1, min_score_rank=1),
    "loop_min_equal_c": lambda: traj(LOOP, 35, 120, 150, 150, win=200, slide=5, conn=3, min_score_rank=4),
    "loop_many_a": lambda: traj(LOOP, 40, 120, 150, 150, win=200, slide=3, nneigh=(0, 2), conn=2, min_score=0.05),
    "loop_many_b": lambda: traj(LOOP, 41, 200, 100, 100, win=130, slide=2, nneigh=(0, 3), conn=4, min_score=0.1),
    "loop_many_c": lambda: traj(LOOP, 42, 64, 80, 80, win=100, slide=2, nneigh=(0, 1), conn=1, min_score=0.2),
    "reloc_many_a": lambda: traj(RELOC, 43, 120, 150, 150, win=200, slide=3, nneigh=(0, 2)),
    "reloc_many_b": lambda: traj(RELOC, 44, 200, 100, 100, win=130, slide=2, nneigh=(0, 3), erased=0.1),
    "loop_all_connected": lambda: traj(LOOP, 36, 12, 64, 64, conn=12),
    "loop_erased_best": lambda: erased_best(LOOP, 37),
    "loop_capacity": lambda: at_capacity(LOOP, 38),
    "loop_query0": lambda: traj(LOOP, 39, 20, 64, 0),
    # maxCommonWords 1, 4, 5 -> minCommonWords 0, 3, 4
    "reloc_max1": lambda: tiny(RELOC, [5, 9, 30], [[5, 7], [8, 9], [30, 31], [1, 2]], neigh=[[1, 2], [0], [3, 1], []], seed=1),
    "reloc_max4": lambda: tiny(RELOC, [1, 2, 3, 4, 5, 6], [[1, 2, 3, 4, 9], [2, 3, 4], [3, 4, 5, 6], [6, 7], [1, 2, 3, 8]],
                               neigh=[[1, 2, 3], [0, 4], [3, 0], [2, 1], [0, 2]], seed=2),
    "reloc_max5": lambda: tiny(RELOC, [1, 2, 3, 4, 5, 6], [[1, 2, 3, 4, 5], [2, 3, 4, 5], [1, 3, 4, 5, 6], [6], [1, 2, 3, 5, 6, 7]],
                               neigh=[[1, 3], [0, 2, 3], [4, 3], [2], [2, 0, 1]], seed=3),
    "loop_max1": lambda: tiny(LOOP, [5, 9, 30], [[5, 7], [8, 9], [30, 31], [1, 2]], neigh=[[1, 2], [0], [3, 1], []], connected=[1], seed=4),
    "loop_max4": lambda: tiny(LOOP, [1, 2, 3, 4, 5, 6], [[1, 2, 3, 4, 9], [2, 3, 4], [3, 4, 5, 6], [6, 7], [1, 2, 3, 8], [1, 2, 3, 4, 5, 6]],
                              neigh=[[1, 2, 3], [0, 4], [3, 0], [2, 1], [0, 2], [0]], connected=[5], min_score=0.01, seed=5),
    "loop_max5": lambda: tiny(LOOP, [1, 2, 3, 4, 5, 6], [[1, 2, 3, 4, 5], [2, 3, 4, 5], [1, 3, 4, 5, 6], [6], [1, 2, 3, 5, 6, 7]],
                              neigh=[[1, 3], [0, 2, 3], [4, 3], [2], [2, 0, 1]], connected=[3], min_score=0.05, seed=6),
    # a query that shares no word with anything
    "reloc_no_share": lambda: tiny(RELOC, [100, 200], [[1, 2], [3, 4], [5]], neigh=[[1], [2], [0]], seed=7),
    "loop_no_share": lambda: tiny(LOOP, [100, 200], [[1, 2], [3, 4], [5]], neigh=[[1], [2], [0]], connected=[0], seed=8),
}
CASES = sorted(_B)
_cache = {}


def case(name):
    """the case's arrays; built once, handed out as they are (treat them as read-only: copy what a call updates)"""
    if name not in _cache:
        _cache[name] = _B[name]()
    return _cache[name]


def digest(c):
    """SHA-256 over the case's input arrays"""
    h = hashlib.sha256()
    h.update(np.int32([c["mode"], c["K"]]).tobytes())
    for key in ("q_word", "q_value", "offsets", "word", "value", "neigh", "connected", "scores"):
        h.update(np.ascontiguousarray(c[key]).tobytes())
    h.update(np.float32(c["min_score"]).tobytes())
    h.update(b"all" if c["active"] is None else c["active"].tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def brute_force_sharing(c):
    """(the sharing list in the reference's order, the common-word count per position): an inverted file written out in Python"""
    K = c["K"]
    connected = set(int(p) for p in c["connected"]) if c["mode"] == LOOP else set()
    inverted = {}
    for k in range(K):
        if c["active"] is not None and not c["active"][k]:
            continue
        for w in c["word"][c["offsets"][k]:c["offsets"][k + 1]]:
            inverted.setdefault(int(w), []).append(k)
    order, count = [], np.zeros(K, np.int32)
    for w in c["q_word"]:
        for k in inverted.get(int(w), []):
            if k in connected:
                continue
            if count[k] == 0:
                order.append(k)
            count[k] += 1
    return order, count
