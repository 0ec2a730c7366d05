"""Timing of the motion-only pose optimization (csrc/pose_optimizer.hip): a batch of 300 problems (about 1 000 observations with a
map point and 2 markers each, tests/pose_opt_cases.problem) through orbfe_pose_optimization_batch_device, the same for one problem,
the host-pointer call end to end, and the CPU restatement (tests/pose_opt_ref.cpp, single thread) on the same problems.
Call times from a host clock around each call plus a blocking download of its result record (median of `reps`, after a
warm-up); prints one JSON line, and writes it to --out.

    python tools/pose_opt_timing.py [--frames 300] [--reps 20] [--out FILE] [--batch-only]
Under rocprofv3 --kernel-trace --stats it gives the launch count per batch call and the kernel time (profiles/)."""
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
import pose_opt_build as B  # noqa: E402
import pose_opt_cases as S  # noqa: E402
from pose_opt_device import Dev  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch-only", action="store_true", help="only the batch call (one kernel shape for a profile)")
    a = ap.parse_args()
    probs = [S.problem(1000, outliers=0.1, nmarkers=2, seed=1000 + f) for f in range(a.frames)]
    F, cap, mcap = len(probs), max(len(p["kps"]) for p in probs), 2
    kps = np.zeros((F, cap), B.KP_DTYPE); has = np.zeros((F, cap), np.uint8); X = np.zeros((F, cap, 3), np.float32)
    mk = np.zeros((F, mcap), B.MARKER_DTYPE); n = np.zeros(F, np.int32); nm = np.zeros(F, np.int32); T = np.zeros((F, 12), np.float32)
    for f, pb in enumerate(probs):
        k = len(pb["kps"])
        kps[f, :k] = pb["kps"]; has[f, :k] = pb["has_mp"]; X[f, :k] = pb["x3Dw"]; mk[f] = pb["markers"]
        n[f] = k; nm[f] = 2; T[f] = pb["Tcw"].reshape(12)
    d = Dev
    d_kps, d_has, d_X, d_mk, d_n, d_nm, d_T = d(kps), d(has), d(X), d(mk), d(n), d(nm), d(T)
    d_To, d_out, d_chi = d(np.zeros_like(T)), d(np.zeros((F, cap), np.uint8)), d(np.zeros((F, cap), np.float32))
    d_res = d(np.zeros(F, binding.POSE_RESULT_DTYPE))

    def run(nframes):
        binding.pose_optimization_batch_device(d_kps.ptr, d_n.ptr, cap, nframes, d_has.ptr, d_X.ptr,
                                               d_mk.ptr, d_nm.ptr, mcap, S.INV_SIGMA2, S.K4, 25.0, d_T.ptr,
                                               d_To.ptr, d_out.ptr, d_chi.ptr, d_res.ptr, None)

    def device_ms(nframes):
        # host clock around one call that ends in a blocking download (the null stream): median over reps
        run(nframes)
        d_res.get()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            run(nframes)
            d_res.get()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    batch_ms = device_ms(F)
    res = d_res.get()
    if a.batch_only:
        print(json.dumps(dict(frames=F, reps=a.reps, batch_device_ms=round(batch_ms, 3))))
        return
    single_ms = device_ms(1)
    pb = probs[0]
    binding.pose_optimization(pb["kps"], pb["has_mp"], pb["x3Dw"], S.INV_SIGMA2, S.K4, pb["Tcw"], markers=pb["markers"])
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        binding.pose_optimization(pb["kps"], pb["has_mp"], pb["x3Dw"], S.INV_SIGMA2, S.K4, pb["Tcw"], markers=pb["markers"])
        ts.append((time.perf_counter() - t0) * 1e3)
    host_call_ms = float(np.median(ts))
    B.pose_optimization(probs[0])
    t0 = time.perf_counter()
    for pb in probs:
        B.pose_optimization(pb)
    ref_ms = (time.perf_counter() - t0) * 1e3
    out = dict(frames=F, capacity=cap, observations_with_map_point=int(has.sum() / F), markers=mcap, reps=a.reps,
               batch_device_ms=round(batch_ms, 3), batch_us_per_problem=round(batch_ms * 1e3 / F, 2),
               single_problem_device_ms=round(single_ms, 3), host_call_ms=round(host_call_ms, 3),
               restatement_cpu_ms_per_problem=round(ref_ms / F, 3), restatement_cpu_ms_batch=round(ref_ms, 1),
               lm_iterations_mean=float(np.mean(res["iterations"][:, :4])), rounds_mean=float(np.mean(res["rounds"])))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
