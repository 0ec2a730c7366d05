"""Timing of the Sim3 RANSAC (csrc/sim3_solver.hip): one 300-iteration solve through the host-pointer call at N = 100 or N = 1000
correspondences, or one orbfe_sim3_solve_batch_device call over 64 problems of N = 1000, and the CPU restatement
(tests/sim3_ref.cpp, one thread) on the same input.  The scenes have no consistent similarity (map 2 shuffled), so that nothing is
found and all 300 iterations run on both sides.  Call times from a host clock around each call
(median of `reps`, after a warm-up); prints one JSON line and writes it to --out.

    python tools/sim3_timing.py --case n100|n1000|batch64 [--reps 20] [--out FILE]
Under rocprofv3 --kernel-trace --stats, one process per case, it gives the kernel times of profiles/sim3_kernel_stats.txt."""
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
import sim3_build as B  # noqa: E402
import sim3_cases as S  # noqa: E402
from pose_opt_device import Dev  # noqa: E402

ITERS = 300


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["n100", "n1000", "batch64"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N = 100 if a.case == "n100" else 1000
    P = 64 if a.case == "batch64" else 1
    scenes = [S.scene(N, 1.3, 0.3, False, seed=50 + p) for p in range(P)]
    words = np.stack([S.words(ITERS, 70 + p) for p in range(P)])
    # the loop closer's (0.99, 20, 300): 300 iterations after clipping at both sizes.  Map 2's points are shuffled, so that no
    # similarity explains the correspondences, no hypothesis exceeds 20 inliers and the restatement runs all 300 iterations too
    min_inl = 20
    for sc in scenes:
        rng = np.random.default_rng(1)
        sc["x3Dw2"] = sc["x3Dw2"][rng.permutation(len(sc["x3Dw2"]))]
    ref = B.solve(scenes[0], 0.99, min_inl, ITERS, words=words[0])
    t0 = time.perf_counter()
    for _ in range(3):
        B.solve(scenes[0], 0.99, min_inl, ITERS, words=words[0])
    ref_ms = (time.perf_counter() - t0) * 1e3 / 3
    out = dict(case=a.case, N=N, problems=P, iterations=ITERS, reps=a.reps, restatement_found=int(ref["result"]["found"]),
               restatement_cpu_ms_per_problem=round(ref_ms, 3))
    if P == 1:
        sc = scenes[0]
        sol = binding.Sim3Solver((sc["kps1"], sc["x3Dw1"], sc["valid1"], sc["Tcw1"], sc["K4_1"]),
                                 (sc["kps2"], sc["x3Dw2"], sc["valid2"], sc["Tcw2"], sc["K4_2"]), sc["m12"], sc["level_sigma2"], False)
        sol.set_ransac_parameters(0.99, min_inl, ITERS)
        ms = _median_ms(lambda: sol.solve(0, ITERS, 0, words[0]), a.reps)
        r, _ = sol.solve(0, ITERS, 0, words[0])
        out.update(host_call_ms=round(ms, 3), found=int(r["found"]), max_iterations=int(r["max_iterations"]))
    else:
        n1 = len(scenes[0]["kps1"])
        cap = n1
        kps = np.zeros((2 * P, cap), binding.KP_DTYPE); x = np.zeros((2 * P, cap, 3), np.float32); v = np.zeros((2 * P, cap), np.uint8)
        T = np.zeros((2 * P, 3, 4), np.float32); nk = np.full(2 * P, n1, np.int32); m12 = np.zeros((P, cap), np.int32)
        for p, sc in enumerate(scenes):
            kps[2 * p], kps[2 * p + 1] = sc["kps1"], sc["kps2"]
            x[2 * p], x[2 * p + 1] = sc["x3Dw1"], sc["x3Dw2"]
            v[2 * p], v[2 * p + 1] = sc["valid1"], sc["valid2"]
            T[2 * p], T[2 * p + 1] = sc["Tcw1"], sc["Tcw2"]
            m12[p] = sc["m12"]
        p1 = np.arange(P, dtype=np.int32) * 2; p2 = p1 + 1
        d = Dev
        d_kps, d_n, d_x, d_v, d_T, d_p1, d_p2, d_m, d_w = d(kps), d(nk), d(x), d(v), d(T), d(p1), d(p2), d(m12), d(words)
        d_res, d_inl = d(np.zeros(P, binding.SIM3_RESULT_DTYPE)), d(np.zeros((P, cap), np.uint8))

        def run():
            binding.sim3_solve_batch_device(d_kps.ptr, d_n.ptr, cap, d_x.ptr, d_v.ptr, d_T.ptr, d_p1.ptr, d_p2.ptr, P, d_m.ptr, S.K4,
                                            S.LEVEL_SIGMA2, False, 0.99, min_inl, ITERS, d_w.ptr, d_res.ptr, d_inl.ptr, None)
            d_res.get()      # blocking: waits for the null stream
        ms = _median_ms(run, a.reps)
        res = d_res.get()
        out.update(batch_call_ms=round(ms, 3), batch_us_per_problem=round(ms * 1e3 / P, 2), found_max=int(res["found"].max()),
                   max_iterations=int(res["max_iterations"].min()))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
