"""Device time of CreateNewMapPoints (csrc/new_map_points.hip), from events on the stream, and the CPU restatement
(tests/new_points_ref.cpp, g++ -O2, one core; the oracle's SearchForTriangulation where the chain searches) on the same host:

    chain-n1000 / chain-n2000   one orbfe_create_new_map_points_device call, 20 neighbours of N features each
    kernels-300                 orbfe_new_points_prepare_batch_device and orbfe_triangulate_matches_batch_device alone, 300 pairs, N = 1000

    python tools/new_points_timing.py [--case chain-n1000|chain-n2000|kernels-300|all] [--reps 20] [--out FILE]

Every figure is the median over `reps` event pairs after a warm-up; the chain's map state is put back between repetitions outside the
timed interval.  Prints one JSON line per case.  Under a kernel-trace-with-stats profiler run of its own it gives the per-kernel table
of profiles/new_map_points_timing.txt."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orb_slam2_aruco_amd import binding  # noqa: E402
import new_points_cases as nc  # noqa: E402

NEIGHBOURS = 20


def cp(a):
    return a.ctypes.data_as(C.c_void_p)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def median_us(fn, reps, reset=None):
    for _ in range(3):
        if reset:
            reset()
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        if reset:
            reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return float(np.median(us)), float(np.min(us)), float(np.max(us))


def check(L, rc):
    if rc != 0:
        raise RuntimeError(L.orbfe_last_error().decode())


def chain_case(N, reps):
    L = binding.load()
    sc = nc.scene(100 + N, N, NEIGHBOURS, baseline=(0.15, 0.4), mapped=0.5, outliers=0.1, shared=False)
    frames = sc["frames"]
    P = nc.pack_frames(frames, N, poison=False)
    pairs = [(0, p) for p in range(1, NEIGHBOURS + 1)]
    d = {k: dev(P[k]) for k in P}
    pristine = {k: d[k].clone() for k in ("x3Dw", "valid", "free")}
    p1, p2 = dev(np.array([a for a, _ in pairs], np.int32)), dev(np.array([b for _, b in pairs], np.int32))
    npairs = len(pairs)
    o = dict(F12=dev(np.zeros((npairs, 9), np.float32)), epi=dev(np.zeros((npairs, 2), np.float32)), prep=dev(np.zeros(npairs, nc.PAIR_DTYPE)),
             m12=dev(np.zeros((npairs, N), np.int32)), s21=dev(np.zeros((npairs, N), np.int32)), nm=dev(np.zeros(npairs, np.int32)),
             status=dev(np.zeros((npairs, N), np.uint8)), x3D=dev(np.zeros((npairs, N, 3), np.float32)), normal=dev(np.zeros((npairs, N, 3), np.float32)),
             dist=dev(np.zeros((npairs, N, 2), np.float32)), res=dev(np.zeros(npairs, nc.RESULT_DTYPE)))
    stream = torch.cuda.current_stream().cuda_stream

    def reset():
        for k, v in pristine.items():
            d[k].copy_(v)

    def run():
        check(L, L.orbfe_create_new_map_points_device(
            d["kps"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr(), d["fn"].data_ptr(), d["fo"].data_ptr(), d["ff"].data_ptr(),
            d["nfv"].data_ptr(), N, d["x3Dw"].data_ptr(), d["valid"].data_ptr(), d["free"].data_ptr(), d["Tcw"].data_ptr(), p1.data_ptr(),
            p2.data_ptr(), npairs, cp(nc.K4), cp(nc.SCALE), cp(nc.SIGMA2), nc.NLEVELS, nc.RATIO, 0, o["F12"].data_ptr(), o["epi"].data_ptr(),
            o["prep"].data_ptr(), o["m12"].data_ptr(), o["s21"].data_ptr(), o["nm"].data_ptr(), o["status"].data_ptr(), o["x3D"].data_ptr(),
            o["normal"].data_ptr(), o["dist"].data_ptr(), o["res"].data_ptr(), stream))

    med, lo, hi = median_us(run, reps, reset)
    res = o["res"].cpu().numpy().view(nc.RESULT_DTYPE)
    nc.ref_sequence(frames[:2])   # builds and loads the restatement and the oracle outside the clock
    t0 = time.perf_counter()
    want, _ = nc.ref_sequence(frames, pairs)
    ref_ms = (time.perf_counter() - t0) * 1e3
    geo = 0.0   # the geometry alone: prepare and triangulation of the lists the sequence found
    for (a, b), w in zip(pairs, want):
        t0 = time.perf_counter()
        nc.ref_prepare(frames[a], frames[b])
        nc.ref_triangulate(frames[a]["kps"], frames[a]["Tcw"], frames[b]["kps"], frames[b]["Tcw"], w["match12"])
        geo += (time.perf_counter() - t0) * 1e3
    same = [int(r["n_new"]) for r in res] == [int(w["result"]["n_new"]) for w in want]
    return dict(case="chain-n%d" % N, N=N, neighbours=NEIGHBOURS, reps=reps, launches=1 + 2 * npairs, device_us_median=round(med, 1),
                device_us_min=round(lo, 1), device_us_max=round(hi, 1), matches=int(res["n_matches"].sum()), new_points=int(res["n_new"].sum()),
                new_points_equal_restatement=bool(same), restatement_with_oracle_search_ms=round(ref_ms, 2),
                restatement_geometry_only_ms=round(geo, 2))


def kernels_case(reps, N=1000, npairs=300):
    L = binding.load()
    sc = nc.scene(77, N, NEIGHBOURS, baseline=(0.15, 0.4), mapped=0.3, outliers=0.1)
    frames = sc["frames"]
    P = nc.pack_frames(frames, N, poison=False)
    pairs = [(0, 1 + p % NEIGHBOURS) for p in range(npairs)]
    lists = [nc.true_matches(sc, f) for f in range(1, NEIGHBOURS + 1)]
    m12 = np.stack([lists[p % NEIGHBOURS] for p in range(npairs)]).astype(np.int32)
    d = {k: dev(P[k]) for k in ("kps", "n", "x3Dw", "valid", "Tcw")}
    p1, p2, dm = dev(np.array([a for a, _ in pairs], np.int32)), dev(np.array([b for _, b in pairs], np.int32)), dev(m12)
    o = dict(F12=dev(np.zeros((npairs, 9), np.float32)), epi=dev(np.zeros((npairs, 2), np.float32)), prep=dev(np.zeros(npairs, nc.PAIR_DTYPE)),
             status=dev(np.zeros((npairs, N), np.uint8)), x3D=dev(np.zeros((npairs, N, 3), np.float32)), normal=dev(np.zeros((npairs, N, 3), np.float32)),
             dist=dev(np.zeros((npairs, N, 2), np.float32)), res=dev(np.zeros(npairs, nc.RESULT_DTYPE)))
    stream = torch.cuda.current_stream().cuda_stream

    def prepare():
        check(L, L.orbfe_new_points_prepare_batch_device(d["n"].data_ptr(), N, d["x3Dw"].data_ptr(), d["valid"].data_ptr(), d["Tcw"].data_ptr(),
                                                         p1.data_ptr(), p2.data_ptr(), npairs, cp(nc.K4), o["F12"].data_ptr(), o["epi"].data_ptr(),
                                                         o["prep"].data_ptr(), stream))

    def triangulate():
        check(L, L.orbfe_triangulate_matches_batch_device(d["kps"].data_ptr(), d["n"].data_ptr(), N, None, None, None, d["Tcw"].data_ptr(),
                                                          p1.data_ptr(), p2.data_ptr(), npairs, dm.data_ptr(), cp(nc.K4), cp(nc.SCALE), cp(nc.SIGMA2),
                                                          nc.NLEVELS, nc.RATIO, o["status"].data_ptr(), o["x3D"].data_ptr(), o["normal"].data_ptr(),
                                                          o["dist"].data_ptr(), o["res"].data_ptr(), stream))

    pm = median_us(prepare, reps)
    tm = median_us(triangulate, reps)
    res = o["res"].cpu().numpy().view(nc.RESULT_DTYPE)
    t0 = time.perf_counter()
    for f in range(1, NEIGHBOURS + 1):
        nc.ref_prepare(frames[0], frames[f])
    ref_prep = (time.perf_counter() - t0) * 1e3 / NEIGHBOURS * npairs
    t0 = time.perf_counter()
    for f in range(1, NEIGHBOURS + 1):
        nc.ref_triangulate(frames[0]["kps"], frames[0]["Tcw"], frames[f]["kps"], frames[f]["Tcw"], lists[f - 1])
    ref_tri = (time.perf_counter() - t0) * 1e3 / NEIGHBOURS * npairs
    return dict(case="kernels-300", N=N, pairs=npairs, reps=reps, matches=int(res["n_matches"].sum()), new_points=int(res["n_new"].sum()),
                prepare_us_median=round(pm[0], 1), prepare_us_min=round(pm[1], 1), prepare_us_max=round(pm[2], 1),
                triangulate_us_median=round(tm[0], 1), triangulate_us_min=round(tm[1], 1), triangulate_us_max=round(tm[2], 1),
                restatement_prepare_ms=round(ref_prep, 2), restatement_triangulate_ms=round(ref_tri, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["chain-n1000", "chain-n2000", "kernels-300", "all"], default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("new_points_timing: no GPU (a timing without one means nothing)")
    lines = []
    for case in (["chain-n1000", "chain-n2000", "kernels-300"] if a.case == "all" else [a.case]):
        r = kernels_case(a.reps) if case == "kernels-300" else chain_case(int(case.split("n")[-1]), a.reps)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
