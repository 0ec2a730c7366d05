"""Timing of OptimizeEssentialGraph (csrc/essential_graph.hip) on one synthetic loop (tests/essential_cases.ring: 1 000 keyframes,
covisibility reach 10, 20 000 points, the last ten keyframes corrected): the device call (the worst case of 20 x 10 trials enqueued,
a host clock around the call and one synchronising fetch), the host call (which stops enqueueing when the control block says so), and
the CPU restatement (tests/essential_ref.cpp, one thread, a dense solve, which is not g2o) on the same input.

The share of the device call spent in launches that fall through: the device call is timed a second time with the iteration cap at
the number of iterations the run takes, so that the two differ by whole iterations of launches that return at once; that gives the cost
of one such launch, and the record says how many of the full call's launches did no work.  Prints one JSON line and writes it to --out.

    python tools/essential_timing.py [--reps 5] [--keyframes 1000] [--out FILE] [--no-gpu | --no-restatement]"""
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
import essential_cases as S  # noqa: E402


def device_call_ms(pb, reps):
    from pose_opt_device import Dev, Out
    a = binding.eg_arrays(pb)
    nkf, ne, n = len(a["Tcw"]), len(a["edge_i"]), len(a["x3Dw"])
    nbytes = binding.essential_graph_scratch_bytes(nkf, ne, n, a["leaf_vertices"])
    ins = {k: Dev(a[k]) for k in ("Tcw", "corrected_pos", "corrected", "noncorrected_pos", "noncorrected", "x3Dw", "point_ref") if a[k].size}
    outs = dict(Tcw_out=Dev(np.zeros((nkf, 12), np.float32)), x3Dw_out=Dev(np.zeros((max(n, 1), 3), np.float32)), Siw_out=Dev(np.zeros((nkf, 8))),
                res=Dev(np.zeros(1, binding.EG_RESULT_DTYPE)), scratch=Dev(np.zeros(nbytes, np.uint8)))
    ptr = {k: v.ptr for k, v in list(ins.items()) + list(outs.items())}
    ptr["scratch_bytes"] = nbytes
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        binding.optimize_essential_graph_device(pb, ptr)
        t1 = time.perf_counter()
        res = outs["res"].get()[0]      # a blocking copy: waits for the null stream
        ts.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
    ts = ts[1:]
    return float(np.median([t[0] for t in ts])), float(np.median([t[1] for t in ts])), res, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    n = a.keyframes
    pb = S.ring(n=n, n_corrected=10, reach=10, n_points=20 * n, rot_step=0.2 / n, trans_step=0.1 / n)
    out = dict(keyframes=n, edges=len(pb["edge_i"]), points=len(pb["x3Dw"]), reps=a.reps)
    if not a.no_gpu:
        g = binding.essential_graph_inspect(dict(pb, x3Dw=np.zeros((0, 3)), point_ref=np.zeros(0)))
        L = int(g["nlevels"])
        out.update(levels=L, nodes=len(g["parent"]), largest_front_rows=int(7 * (g["nown"] + g["nb"]).max()))
        binding.optimize_essential_graph(pb)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = binding.optimize_essential_graph(pb)
            ts.append((time.perf_counter() - t0) * 1e3)
        res = r["result"]
        k, trials = int(res["iterations"]), int(res["trials"])
        out.update(host_call_ms=round(float(np.median(ts)), 3), iterations=k, trials=trials, chi2_first=float(res["chi2_first"]), chi2_last=float(res["chi2_last"]))
        full, enq, dres, nbytes = device_call_ms(pb, a.reps)
        short, _, _, _ = device_call_ms(dict(pb, iterations=k), a.reps)
        per_trial = 2 * L - 1 + 3
        per_iteration = 3 + 10 * per_trial
        launches = 3 + 20 * per_iteration + 1
        worked = 3 + k * 3 + trials * per_trial + 1
        per_launch_us = (full - short) * 1e3 / max((20 - k) * per_iteration, 1)
        out.update(scratch_mb=round(nbytes / 2 ** 20, 1), device_call_ms=round(full, 3), device_call_enqueue_ms=round(enq, 3),
                   device_call_capped_at_iterations_run_ms=round(short, 3), launches=launches, launches_that_worked=worked,
                   fall_through_launch_us=round(per_launch_us, 2), fall_through_share=round(per_launch_us * 1e-3 * (launches - worked) / full, 3),
                   device_equals_host=bool(dres.tobytes() == res.tobytes()))
    if not a.no_restatement:
        import essential_build as B
        t0 = time.perf_counter()
        ref = B.optimize(pb)
        out.update(restatement_cpu_ms=round((time.perf_counter() - t0) * 1e3, 1), restatement_iterations=ref["result"]["iterations"],
                   restatement_trials=ref["result"]["trials"])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
