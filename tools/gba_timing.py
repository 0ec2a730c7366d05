"""Timing of GlobalBundleAdjustment (csrc/global_ba.hip) on two inputs: a synthetic loop (tests/gba_cases.track: 1 000 keyframes on
a ring, 20 000 points seen from 4 - 6 consecutive keyframes each, some 10^5 observations, 10 iterations without Huber: the loop-closing
call) and the local bundle adjustment's timing input (tests/lba_cases.timing_problem: 40 keyframes, 3 000 points, 2 markers).  For each:
the host call (which stops enqueueing when the control block says so), the device call (the worst case of iterations x 10 trials
enqueued, a host clock around the call and one synchronising fetch), and the share of the device call's launches that fall through:
the device call is timed a second time with the iteration cap at the number of iterations the run takes, so that the two differ by
whole iterations of launches that return at once.  The CPU restatement (tests/gba_ref.cpp, one thread, a DENSE reduced solve, which
is not g2o) runs on the same machine on the 40-keyframe input, and on the loop with --restatement-loop (minutes: 6 000 dense rows).

Per-kernel times come from a profiler run of one host call:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gba_timing.py --one-call
Prints one JSON line and writes it to --out.

    python tools/gba_timing.py [--reps 5] [--keyframes 1000] [--out FILE] [--no-gpu | --no-restatement] [--restatement-loop] [--one-call]"""
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
import gba_cases as S  # noqa: E402
import lba_cases  # noqa: E402


def loop(nkf):
    return dict(S.track(nkf, 20 * nkf, 61, span=(4, 6), ring=True), iterations=10, robust=0)


def device_call_ms(pb, reps):
    from pose_opt_device import Dev
    a = binding.gba_arrays(pb)
    nkf, n, nobs, nma, nmobs = len(a["Tcw"]), len(a["x3Dw"]), len(a["obs_kf"]), len(a["Twm"]), len(a["mobs_kf"])
    nbytes = binding.gba_scratch_bytes(nkf, n, nobs, nma, nmobs, a["leaf_vertices"])
    d = {k: Dev(a[k]) for k in ("Tcw", "x3Dw", "obs_xy", "obs_octave", "Twm", "marker_local", "mobs_corners") if a[k].size}
    d.update(res=Dev(np.zeros(1, binding.GBA_RESULT_DTYPE)), scratch=Dev(np.zeros(nbytes, np.uint8)))
    ptr = {k: v.ptr for k, v in d.items()}
    ptr["scratch_bytes"] = nbytes
    ts = []
    for _ in range(reps + 1):
        for k in ("Tcw", "x3Dw", "Twm"):       # in place: every repeat starts from the same estimates
            if k in d:
                d[k].put(a[k])
        t0 = time.perf_counter()
        binding.global_bundle_adjustment_device(pb, ptr)
        t1 = time.perf_counter()
        res = d["res"].get()[0]      # a blocking copy: waits for the null stream
        ts.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
    ts = ts[1:]
    return float(np.median([t[0] for t in ts])), float(np.median([t[1] for t in ts])), res, nbytes


def measure(pb, reps, gpu, restatement):
    out = dict(keyframes=len(pb["Tcw"]), points=len(pb["x3Dw"]), observations=len(pb["obs_kf"]), markers=len(pb["Twm"]), iterations_asked=pb["iterations"],
               robust=pb["robust"])
    if gpu:
        g = binding.gba_inspect(pb)
        L = int(g["nlevels"])
        out.update(free_vertices=g["nv"], levels=L, nodes=len(g["parent"]), largest_front_rows=int(6 * (g["nown"] + g["nb"]).max()))
        binding.global_bundle_adjustment(pb)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = binding.global_bundle_adjustment(pb)
            ts.append((time.perf_counter() - t0) * 1e3)
        res = r["result"]
        k, trials = int(res["iterations"]), int(res["trials"])
        out.update(host_call_ms=round(float(np.median(ts)), 3), iterations=k, trials=trials, chi2_first=float(res["chi2_first"]), chi2_last=float(res["chi2_last"]))
        full, enq, dres, nbytes = device_call_ms(pb, reps)
        short, _, _, _ = device_call_ms(dict(pb, iterations=k), reps)
        per_trial = 5 + L + max(L - 1, 0)
        per_iteration = 3 + 10 * per_trial
        launches = 2 + pb["iterations"] * per_iteration + 1
        worked = 2 + k * 3 + trials * per_trial + 1
        idle = (pb["iterations"] - k) * per_iteration      # launches of whole iterations that fall through; none when every iteration ran
        per_launch_us = (full - short) * 1e3 / idle if idle else None
        out.update(scratch_mb=round(nbytes / 2 ** 20, 1), device_call_ms=round(full, 3), device_call_enqueue_ms=round(enq, 3),
                   device_call_capped_at_iterations_run_ms=round(short, 3), launches=launches, launches_that_worked=worked,
                   share_of_launches_falling_through=round(1 - worked / launches, 3), fall_through_launch_us=None if per_launch_us is None else round(per_launch_us, 2),
                   device_equals_host=bool(dres.tobytes() == res.tobytes()))
    if restatement:
        import gba_build
        gba_build.lib()
        t0 = time.perf_counter()
        r = gba_build.global_bundle_adjustment(pb, gba_build.INSERTION)
        out.update(restatement_one_core_dense_ms=round((time.perf_counter() - t0) * 1e3, 1), restatement_iterations=int(r["result"]["iterations"]),
                   restatement_note="tests/gba_ref.cpp on one core with a dense reduced solve: not g2o")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--restatement-loop", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--one-call", action="store_true", help="one warm-up and one host call on the loop, for a profiler run")
    a = ap.parse_args()
    big = loop(a.keyframes)
    if a.one_call:
        binding.global_bundle_adjustment(big)
        r = binding.global_bundle_adjustment(big)
        print(json.dumps(dict(iterations=int(r["result"]["iterations"]), trials=int(r["result"]["trials"]))))
        return
    small = dict(lba_cases.timing_problem(), iterations=10, robust=0)
    out = dict(reps=a.reps,
               loop=measure(big, a.reps, not a.no_gpu, a.restatement_loop and not a.no_restatement),
               lba_input=measure(small, a.reps, not a.no_gpu, not a.no_restatement))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
