"""Timing of OptimizeSim3 (csrc/sim3_optimizer.hip): one problem through the host-pointer call at N = 100 or N = 1000 correspondences
(30 % gross outliers, 1 px of noise, free scale: tests/sim3_opt_cases.problem), or one orbfe_optimize_sim3_batch_device call over 64
problems of N = 1000, and the CPU restatement (tests/sim3_opt_ref.cpp, one thread) on the same input.  Call times from a host
clock around each call (median of `reps`, after a warm-up); prints one JSON line and writes it to --out.

    python tools/sim3_opt_timing.py --case n100|n1000|batch64 [--reps 20] [--out FILE]
Under a kernel-trace-with-stats profiler run of its own, one process per case, it gives the kernel times of
profiles/sim3_opt_kernel_stats.txt."""
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
import sim3_cases  # noqa: E402
import sim3_opt_build as B  # noqa: E402
import sim3_opt_cases as S  # noqa: E402
from pose_opt_device import Dev  # noqa: E402


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
    probs = [S.problem(N, 1.3, 0.3, False, True, 1.0, seed=50 + p) for p in range(P)]
    ref = B.optimize_sim3(probs[0])["result"]
    t0 = time.perf_counter()
    for _ in range(3):
        B.optimize_sim3(probs[0])
    ref_ms = (time.perf_counter() - t0) * 1e3 / 3
    out = dict(case=a.case, N=N, problems=P, reps=a.reps, restatement_inliers=int(ref["n_inliers"]),
               restatement_lm_iterations=ref["iterations"].tolist(), restatement_cpu_ms_per_problem=round(ref_ms, 3))

    def host_call(pb):
        return binding.optimize_sim3((pb["kps1"], pb["x3Dw1"], pb["valid1"], pb["Tcw1"], pb["K4_1"]),
                                     (pb["kps2"], pb["x3Dw2"], pb["valid2"], pb["Tcw2"], pb["K4_2"]), pb["m12"], pb["inv_sigma2"],
                                     pb["s12_0"], pb["R12_0"], pb["t12_0"], pb["th2"], pb["fix_scale"])
    if P == 1:
        ms = _median_ms(lambda: host_call(probs[0]), a.reps)
        _, r = host_call(probs[0])
        out.update(host_call_ms=round(ms, 3), inliers=int(r["n_inliers"]), lm_iterations=r["iterations"].tolist())
    else:
        cap = len(probs[0]["kps1"])
        kps = np.zeros((2 * P, cap), binding.KP_DTYPE); x = np.zeros((2 * P, cap, 3), np.float32); v = np.zeros((2 * P, cap), np.uint8)
        T = np.zeros((2 * P, 3, 4), np.float32); nk = np.full(2 * P, cap, np.int32); m12 = np.zeros((P, cap), np.int32)
        sim = np.zeros((P, 13), np.float32)
        for p, pb in enumerate(probs):
            kps[2 * p], kps[2 * p + 1] = pb["kps1"], pb["kps2"]
            x[2 * p], x[2 * p + 1] = pb["x3Dw1"], pb["x3Dw2"]
            v[2 * p], v[2 * p + 1] = pb["valid1"], pb["valid2"]
            T[2 * p], T[2 * p + 1] = pb["Tcw1"], pb["Tcw2"]
            m12[p] = pb["m12"]
            sim[p] = np.r_[pb["s12_0"], pb["R12_0"].ravel(), pb["t12_0"]]
        p1 = np.arange(P, dtype=np.int32) * 2; p2 = p1 + 1
        d = Dev
        d_kps, d_n, d_x, d_v, d_T, d_p1, d_p2, d_m, d_sim = d(kps), d(nk), d(x), d(v), d(T), d(p1), d(p2), d(m12), d(sim)
        d_out, d_res = d(np.zeros((P, cap), np.int32)), d(np.zeros(P, binding.SIM3_OPT_RESULT_DTYPE))

        def run():
            binding.optimize_sim3_batch_device(d_kps.ptr, d_n.ptr, cap, d_x.ptr, d_v.ptr, d_T.ptr, d_p1.ptr, d_p2.ptr, P, d_m.ptr,
                                               sim3_cases.K4, S.INV_SIGMA2, d_sim.ptr, 52, S.TH2, False, d_out.ptr, d_res.ptr, None)
            d_res.get()      # blocking: waits for the null stream
        ms = _median_ms(run, a.reps)
        res = d_res.get()
        out.update(batch_call_ms=round(ms, 3), batch_us_per_problem=round(ms * 1e3 / P, 2), inliers_mean=float(res["n_inliers"].mean()),
                   lm_iterations_mean=float(res["iterations"].sum(1).mean()))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
