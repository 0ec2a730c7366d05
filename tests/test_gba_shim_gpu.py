"""GPU: include/shims/Optimizer_globalba_orbfe.cc, built with g++ against the mock headers, runs Optimizer::BundleAdjustment on the
hand-built map of tests/gba_shim_map.py and leaves in the map what the C ABI returns for the collected problem, bit for bit, in both
nLoopKF branches: SetPose / SetWorldPos + UpdateNormalAndDepth, or mTcwGBA / mPosGBA / mnBAGlobalForKF; the markers in both."""
import subprocess

import numpy as np
import pytest

import gba_build
import gba_shim_map as M

pytestmark = pytest.mark.gpu


def _run(exe, tmp_path, m, use, stop, nloop, iterations, robust):
    pre, post = str(tmp_path / "in"), str(tmp_path / ("out%d%d%d" % (use, stop, nloop)))
    M.write(m, pre)
    subprocess.check_call([exe, "run", pre, post, str(use), str(stop), str(nloop), str(iterations), str(robust)])
    nk, npt = len(m["kfs"]), len(m["mps"])
    counts = np.fromfile(post + "_counts.bin", np.int32).reshape(-1, 2)
    rd = lambda name, shape: np.fromfile(post + "_" + name + ".bin", np.float32).reshape(shape)
    return dict(T=rd("T", (nk, 4, 4)), Tg=rd("Tg", (nk, 4, 4)), P=rd("P", (npt, 3)), Pg=rd("Pg", (npt, 3)), M=rd("M", (-1, 3, 4)),
                set_pose=counts[:nk, 0], kf_tag=counts[:nk, 1], updates=counts[nk:, 0], mp_tag=counts[nk:, 1])


def test_shim_applies_what_the_binding_returns_in_both_branches(orbfe, tmp_path):
    exe = gba_build.build_shim(str(tmp_path))
    m = M.build()
    kfs, mps, mas = m["kfs"], m["mps"], m["mas"]
    for use, nloop, iterations, robust in ((1, 0, 20, 1), (1, 7, 10, 0), (0, 0, 10, 0)):
        got = _run(exe, tmp_path, m, use, 0, nloop, iterations, robust)
        pb, vertices, points, markers = M.collect(m, use_markers=bool(use))
        want = orbfe.global_bundle_adjustment(dict(pb, iterations=iterations, robust=robust))
        assert want["result"]["status"] == 0 and want["result"]["n_points_left_out"] == 1 and want["result"]["n_edges_marker"] == (20 if use else 0)
        rest = [k for k in range(len(kfs)) if k not in vertices]
        others = [p for p in range(len(mps)) if p not in points or p == m["edgeless"]]
        assert len(rest) == 2 and len(others) == 2
        for i, k in enumerate(vertices):
            new = got["T"][k] if nloop == 0 else got["Tg"][k]
            assert new[:3].tobytes() == want["Tcw"][i].tobytes() and np.array_equal(new[3], [0, 0, 0, 1])
            assert got["set_pose"][k] == (1 if nloop == 0 else 0) and got["kf_tag"][k] == nloop
            if nloop:
                assert np.array_equal(got["T"][k][:3], kfs[k]["T"])
        assert all(got["set_pose"][k] == 0 and got["kf_tag"][k] == 0 and np.array_equal(got["T"][k][:3], kfs[k]["T"]) and (got["Tg"][k] == -1).all() for k in rest)
        assert sum(not np.array_equal(want["Tcw"][i], pb["Tcw"][i]) for i in range(len(vertices))) == 5
        for j, p in enumerate(points):
            if p == m["edgeless"]:
                continue
            new = got["P"][p] if nloop == 0 else got["Pg"][p]
            assert new.tobytes() == want["x3Dw"][j].tobytes() and got["updates"][p] == (1 if nloop == 0 else 0) and got["mp_tag"][p] == nloop
            if nloop:
                assert np.array_equal(got["P"][p], mps[p]["X"])
        assert all(got["updates"][p] == 0 and got["mp_tag"][p] == 0 and np.array_equal(got["P"][p], mps[p]["X"]) and (got["Pg"][p] == -1).all() for p in others)
        # markers: written with mbUArucoIni, in the nLoopKF branch as well
        for a in range(len(mas)):
            old = np.asarray(mas[a]["Twm"], np.float32)
            assert got["M"][a].tobytes() == (want["Twm"][markers.index(a)] if a in markers else old).tobytes()
        if use:
            assert not np.array_equal(got["M"][0], np.asarray(mas[0]["Twm"], np.float32))
    # *pbStopFlag set at the call: nothing is touched
    got = _run(exe, tmp_path, m, 1, 1, 7, 10, 0)
    assert not got["set_pose"].any() and not got["kf_tag"].any() and not got["mp_tag"].any() and (got["Tg"] == -1).all() and (got["Pg"] == -1).all()
    assert all(np.array_equal(got["T"][k][:3], kfs[k]["T"]) for k in range(len(kfs))) and all(np.array_equal(got["P"][p], mps[p]["X"]) for p in range(len(mps)))
