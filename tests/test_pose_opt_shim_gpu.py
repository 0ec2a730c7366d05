"""GPU: include/shims/Optimizer_pose_orbfe.cc, built with g++ against the mock headers of tests/mock_orbslam/, runs one frame with map
points and mapped markers (plus an old and a bad marker that must be left out) through Optimizer::PoseOptimizationByAruco and
returns what the C ABI returns for the same inputs, bit for bit; PoseOptimization throws on a stereo observation."""
import subprocess

import numpy as np
import pytest

import pose_opt_cases as S
import shim_build

pytestmark = pytest.mark.gpu


def test_pose_shim_equals_the_binding(orbfe, tmp_path):
    exe = shim_build.build("pose", str(tmp_path))
    pb = S.case("n500_out10_m3")
    rng = np.random.default_rng(0)
    out0 = (rng.random(len(pb["kps"])) < 0.3).astype(np.uint8)   # mvbOutlier before the call: overwritten where there is a map point
    pre, post = str(tmp_path / "in"), str(tmp_path / "out")
    pb["kps"].tofile(pre + "_kps.bin"); pb["has_mp"].tofile(pre + "_has.bin"); pb["x3Dw"].astype(np.float32).tofile(pre + "_x.bin")
    pb["inv_sigma2"].tofile(pre + "_sig.bin"); pb["K4"].tofile(pre + "_K.bin"); pb["markers"].tofile(pre + "_mk.bin")
    pb["Tcw"].astype(np.float32).tofile(pre + "_T.bin"); out0.tofile(pre + "_out.bin")
    subprocess.check_call([exe, pre, post, repr(S.MARKER_SIDE)])
    T = np.fromfile(post + "_T.bin", np.float32).reshape(4, 4)
    out = np.fromfile(post + "_out.bin", np.uint8)
    ret = int(np.fromfile(post + "_ret.bin", np.int32)[0])
    wT, wout, _, wres = orbfe.pose_optimization(pb["kps"], pb["has_mp"], pb["x3Dw"], pb["inv_sigma2"], pb["K4"], pb["Tcw"],
                                                markers=pb["markers"], outlier=out0.copy())
    assert ret == wres["n_good"] and wres["n_marker_edges"] == 12
    assert T[:3].tobytes() == wT.tobytes() and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.array_equal(out, wout)
    assert int(np.fromfile(post + "_threw.bin", np.int32)[0]) == 1
