"""Timing of the KeyFrameDatabase candidate queries (csrc/keyframe_db.hip): one resident database of K keyframes of about `words` words
each -- four fifths of a keyframe's words from a window that slides along the trajectory, one fifth from a pool every keyframe draws
from, so that every keyframe shares some word with every query -- queried through orbfe_detect_candidates_batch_device with nq = 1
and nq = 64, and through the host-pointer call, which uploads the database on every query.  The three are timed in turn, `reps`
rounds after a warm-up round, with a host clock around each call up to the blocking download of the result records; the CPU
restatement (tests/kfdb_ref.cpp, one thread) runs the first 16 of the same queries with a host clock around each query (its keyframes
and inverted file are built once, before the clock starts, as the reference holds them ready).  Prints one JSON line (median, and the 10th / 90th percentile as the spread) and
writes it to --out.

    python tools/kfdb_timing.py [--mode reloc|loop] [--K 2000] [--words 1000] [--reps 30] [--only CALL] [--out FILE]
Under a kernel-trace-with-stats profiler run of its own, with --only, it gives the kernel times of profiles/kfdb_kernel_stats.txt."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from orb_slam2_aruco_amd import binding  # noqa: E402
import kfdb_build as B  # noqa: E402
import kfdb_cases as S  # noqa: E402
from pose_opt_device import Dev  # noqa: E402

NQ = 64


def database(K, words, seed=1):
    rng = np.random.default_rng(seed)
    local, shared = words * 4 // 5, words - words * 4 // 5
    win, slide = 2 * local, max(1, local // 4)
    pool = np.sort(rng.choice(1 << 20, size=(K + 1) * slide + win + 25 * shared, replace=False))
    everyone, track = pool[:25 * shared], pool[25 * shared:]

    def bow(at):
        w = np.sort(np.concatenate([rng.choice(track[at * slide:at * slide + win], local, replace=False), rng.choice(everyone, shared, replace=False)]))
        v = rng.random(len(w)) + 0.05
        return w.astype(np.uint32), v / v.sum()
    bows = [bow(k) for k in range(K)]
    queries = [bow(int(rng.integers(0, K))) for _ in range(NQ)]
    neigh = np.full((K, 10), -1, np.int32)
    for k in range(K):
        near = [p for p in range(k - 8, k + 9) if p != k and 0 <= p < K]
        row = rng.permutation(near)[:10]
        neigh[k, :len(row)] = row
    return bows, queries, neigh


def stats(ts):
    ts = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), p10_ms=round(float(np.percentile(ts, 10)), 4), p90_ms=round(float(np.percentile(ts, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["reloc", "loop"], default="reloc")
    ap.add_argument("--K", type=int, default=2000)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", choices=["batch_nq1", "batch_nq64", "host_call"], default=None, help="time this call alone (a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mode = S.RELOC if a.mode == "reloc" else S.LOOP
    K, cap = a.K, a.words
    bows, queries, neigh = database(K, a.words)
    rng = np.random.default_rng(2)
    conn = [np.sort(rng.choice(K, 15, replace=False)).astype(np.int32) for _ in range(NQ)]
    min_score = np.full(NQ, 0.02, np.float32)
    state = np.zeros((NQ, K), np.float32)
    cases = [S._finish(mode, q, bows, None, neigh, conn[i] if mode == S.LOOP else [], min_score[i], state[i]) for i, q in enumerate(queries)]
    # the CPU restatement: the database built once, the clock around each of the first 16 queries
    ref_db = B.Database(cases[0])
    cpu, want = [], []
    for c in cases[:16]:
        sc = c["scores"].copy()
        t0 = time.perf_counter()
        r = ref_db.query(c, sc)
        cpu.append(time.perf_counter() - t0)
        want.append(r)
    # the block layout of the vocabulary transform: frames 0 .. K-1 the database, K .. K + NQ - 1 the queries
    bw, bv = np.zeros((K + NQ, cap), np.uint32), np.zeros((K + NQ, cap))
    for f, (w, v) in enumerate(bows + queries):
        bw[f, :len(w)], bv[f, :len(w)] = w, v
    nb = np.full(K + NQ, cap, np.int32)
    off = np.zeros(NQ + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in conn])
    d = Dev
    d_bw, d_bv, d_nb, d_ng, d_q = d(bw), d(bv), d(nb), d(neigh), d(np.arange(K, K + NQ, dtype=np.int32))
    d_co, d_c, d_ms = d(off), d(np.concatenate(conn)), d(min_score)
    d_sc, d_cand, d_com, d_scr = d(state), d(np.zeros((NQ, K), np.int32)), d(np.zeros((NQ, K), np.int32)), d(np.zeros((NQ, K), np.uint32))
    d_res = d(np.zeros(NQ, binding.KFDB_RESULT_DTYPE))

    def batch(nq):
        binding.detect_candidates_batch_device(mode, d_bw.ptr, d_bv.ptr, d_nb.ptr, cap, None, None, K, d_q.ptr, nq, d_ng.ptr, d_co.ptr, d_c.ptr,
                                               d_ms.ptr, d_sc.ptr, d_cand.ptr, d_com.ptr, d_scr.ptr, d_res.ptr, None)
        return d_res.get()      # blocking: waits for the null stream

    def host():
        c = cases[0]
        return binding.detect_candidates(mode, c["q_word"], c["q_value"], c["offsets"], c["word"], c["value"], c["neigh"], c["scores"].copy(),
                                         connected=c["connected"], min_score=c["min_score"])
    runs = dict(batch_nq1=lambda: batch(1), batch_nq64=lambda: batch(NQ), host_call=host)
    if a.only:
        runs = {a.only: runs[a.only]}
    times = {k: [] for k in runs}
    for rep in range(a.reps + 1):      # the three in turn; the first round is the warm-up
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                times[k].append(time.perf_counter() - t0)
    res, cand = batch(NQ), d_cand.get()
    for i, w in enumerate(want):        # the timed work is the right work
        assert res[i].tobytes() == w["result"].tobytes() and np.array_equal(cand[i, :res[i]["n_candidates"]], w["candidates"]), i
    out = dict(mode=a.mode, K=K, words=a.words, reps=a.reps, n_sharing_mean=float(res["n_sharing"].mean()), n_scored_mean=float(res["n_scored"].mean()),
               n_candidates_mean=float(res["n_candidates"].mean()), cpu_restatement_query=stats(cpu),
               **{k: stats(v) for k, v in times.items()})
    if "batch_nq64" in out:
        out["batch_nq64_us_per_query"] = round(out["batch_nq64"]["median_ms"] * 1e3 / NQ, 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
