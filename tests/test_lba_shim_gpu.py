"""GPU: include/shims/Optimizer_localba_orbfe.cc, built with g++ against the mock headers of
tests/mock_orbslam/, runs Optimizer::LocalBundleAdjustment on the hand-built map of tests/lba_shim_map.py and leaves in the map what
the C ABI returns for the collected problem, bit for bit: erased observations, poses, points, marker poses."""
import subprocess

import numpy as np
import pytest

import lba_build
import lba_shim_map as M

pytestmark = pytest.mark.gpu


def _run(exe, tmp_path, m, use, stop):
    pre, post = str(tmp_path / "in"), str(tmp_path / ("out%d%d" % (use, stop)))
    M.write(m, pre)
    subprocess.check_call([exe, "run", pre, post, str(use), str(stop)])
    nk, npt = len(m["kfs"]), len(m["mps"])
    counts = np.fromfile(post + "_counts.bin", np.int32)
    return dict(T=np.fromfile(post + "_T.bin", np.float32).reshape(nk, 4, 4), P=np.fromfile(post + "_P.bin", np.float32).reshape(npt, 3),
                M=np.fromfile(post + "_M.bin", np.float32).reshape(-1, 3, 4), set_pose=counts[:nk], updates=counts[nk:],
                present=np.fromfile(post + "_present.bin", np.int32))


def test_shim_applies_what_the_binding_returns(orbfe, tmp_path):
    exe = lba_build.build_shim(str(tmp_path))
    m = M.build()
    kfs, mps, mas = m["kfs"], m["mps"], m["mas"]
    obs = [(i, k) for i, p in enumerate(mps) for k, _ in sorted(p["obs"].items())]
    for use in (1, 0):
        got = _run(exe, tmp_path, m, use, 0)
        pb, vertices, nlocal, points, markers, edges = M.collect(m, use_markers=bool(use))
        want = orbfe.local_bundle_adjustment(pb)
        assert want["result"]["status"] == 0 and want["result"]["n_erase"] > 0 and want["result"]["n_edges_marker"] == (20 if use else 0)
        # keyframes: every local one received its pose (the mnId 0 one its own), nobody else was touched
        for i, k in enumerate(vertices):
            assert got["T"][k][:3].tobytes() == want["Tcw"][i].tobytes() and np.array_equal(got["T"][k][3], [0, 0, 0, 1])
            assert got["set_pose"][k] == (1 if i < nlocal else 0)
        rest = [k for k in range(len(kfs)) if k not in vertices]
        assert all(got["set_pose"][k] == 0 and np.array_equal(got["T"][k][:3], kfs[k]["T"]) for k in rest)
        moved = [i for i, k in enumerate(vertices) if i < nlocal and kfs[k]["id"] != 0]
        assert all(not np.array_equal(want["Tcw"][i], pb["Tcw"][i]) for i in moved)
        zero = [i for i, k in enumerate(vertices) if kfs[k]["id"] == 0]
        assert len(zero) == 1 and np.array_equal(want["Tcw"][zero[0]], pb["Tcw"][zero[0]])
        # points: the local ones moved and were updated once, the others (the bad one) were not
        for j, p in enumerate(points):
            assert got["P"][p].tobytes() == want["x3Dw"][j].tobytes() and got["updates"][p] == 1
        others = [p for p in range(len(mps)) if p not in points]
        assert others and all(got["updates"][p] == 0 and np.array_equal(got["P"][p], mps[p]["X"]) for p in others)
        # markers: written with mbUArucoIni only
        for j, a in enumerate(markers):
            assert got["M"][a].tobytes() == (want["Twm"][j] if use else np.asarray(mas[a]["Twm"], np.float32)).tobytes()
        assert np.array_equal(got["M"][2], np.asarray(mas[2]["Twm"], np.float32))
        # the erase list: exactly those (keyframe, point) pairs lost both the match and the observation
        erased = set(e for e, flag in zip(edges, want["erase"]) if flag)
        for (i, k), present in zip(obs, got["present"]):
            assert present == (0 if (k, i) in erased else 3), (i, k, present)
    # *pbStopFlag set at the call: nothing is touched
    got = _run(exe, tmp_path, m, 1, 1)
    assert not got["set_pose"].any() and not got["updates"].any() and (got["present"] == 3).all()
    assert all(np.array_equal(got["T"][k][:3], kfs[k]["T"]) for k in range(len(kfs)))
