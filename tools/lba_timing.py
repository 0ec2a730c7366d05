"""Timing of LocalBundleAdjustment (csrc/local_ba.hip) on a local-mapping sized problem (tests/lba_cases.timing_problem: 20 free and
20 fixed keyframes, 3 000 points, 2 markers, 10 % gross outliers): the host-pointer call end to end from a host clock around it
(median of `reps` after a warm-up) and the CPU restatement (tests/lba_ref.cpp, one
thread, which is not g2o) on the same input.  Prints one JSON line and writes it to --out.

    python tools/lba_timing.py [--reps 10] [--out FILE]
Under a kernel-trace-with-stats profiler run of its own it gives the kernel times of profiles/lba_kernel_stats.txt."""
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
import lba_build as B  # noqa: E402
import lba_cases as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    pb = S.timing_problem()
    arr = binding.lba_arrays(pb)
    out = dict(keyframes=len(arr["Tcw"]), free_keyframes=int((arr["kf_fixed"] == 0).sum()), points=len(arr["x3Dw"]), edges_mono=len(arr["obs_kf"]),
               edges_marker=4 * len(arr["mobs_kf"]), reps=a.reps,
               scratch_mb=round(binding.lba_scratch_bytes(len(arr["Tcw"]), len(arr["x3Dw"]), len(arr["obs_kf"]), len(arr["Twm"]), len(arr["mobs_kf"])) / 2 ** 20, 1))
    if not a.no_restatement:
        t0 = time.perf_counter()
        ref = B.local_bundle_adjustment(pb, B.INSERTION)
        out.update(restatement_cpu_ms=round((time.perf_counter() - t0) * 1e3, 1), restatement_iterations=ref["result"]["iterations"].tolist(),
                   restatement_n_erase=int(ref["result"]["n_erase"]))
    binding.local_bundle_adjustment(pb)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = binding.local_bundle_adjustment(pb)
        ts.append((time.perf_counter() - t0) * 1e3)
    res = r["result"]
    out.update(host_call_ms=round(float(np.median(ts)), 3), host_call_ms_min=round(min(ts), 3), host_call_ms_max=round(max(ts), 3),
               iterations=res["iterations"].tolist(), n_level1=res["n_level1"].tolist(), n_erase=int(res["n_erase"]))
    if not a.no_restatement:
        out["erase_equal_to_restatement"] = bool(np.array_equal(r["erase"], ref["erase"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
