"""GPU: include/shims/Optimizer_sim3_orbfe.cc, built with g++ against the mock headers of tests/mock_orbslam/, runs one scene the way
LoopClosing::ComputeSim3 does and returns what the C ABI returns for the same inputs through binding.optimize_sim3 -- fed the
similarity as the shim rounds it to float (the driver dumps it, tests/sim3_opt_shim_driver.cpp)."""
import subprocess

import numpy as np
import pytest

import sim3_opt_cases as S
import shim_build

pytestmark = pytest.mark.gpu


def test_optimize_sim3_shim_returns_the_bindings_result(orbfe, tmp_path):
    exe = shim_build.build("sim3_opt", str(tmp_path))
    pb = S.case("n257_out30")
    p = str(tmp_path / "in")
    pb["kps1"].tofile(p + "_kps1.bin"); pb["kps2"].tofile(p + "_kps2.bin")
    pb["x3Dw1"].tofile(p + "_x1.bin"); pb["x3Dw2"].tofile(p + "_x2.bin")
    pb["valid1"].tofile(p + "_v1.bin"); pb["valid2"].tofile(p + "_v2.bin")
    pb["m12"].astype(np.int32).tofile(p + "_m12.bin")
    pb["Tcw1"].tofile(p + "_T1.bin"); pb["Tcw2"].tofile(p + "_T2.bin")
    pb["K4_1"].tofile(p + "_K.bin"); pb["inv_sigma2"].tofile(p + "_is2.bin")
    np.r_[pb["s12_0"], pb["R12_0"].ravel(), pb["t12_0"]].astype(np.float32).tofile(p + "_sim.bin")
    np.array([pb["th2"], float(pb["fix_scale"])], np.float32).tofile(p + "_par.bin")
    out = str(tmp_path / "out")
    subprocess.run([exe, p, out], check=True, timeout=120)
    ci = np.fromfile(out + "_i.bin", np.int32)
    cd = np.fromfile(out + "_d.bin", np.float64)
    sim = np.fromfile(out + "_sim.bin", np.float32)
    assert np.abs(sim - np.r_[pb["s12_0"], pb["R12_0"].ravel(), pb["t12_0"]]).max() < 1e-6
    m12, res = orbfe.optimize_sim3((pb["kps1"], pb["x3Dw1"], pb["valid1"], pb["Tcw1"], pb["K4_1"]),
                                   (pb["kps2"], pb["x3Dw2"], pb["valid2"], pb["Tcw2"], pb["K4_2"]), pb["m12"], pb["inv_sigma2"],
                                   sim[0], sim[1:10], sim[10:13], pb["th2"], pb["fix_scale"])
    assert res["n_inliers"] > 100 and res["n_bad"] > 0
    assert ci[0] == res["n_inliers"]
    assert np.array_equal(ci[1:] != 0, m12 >= 0)           # NULL exactly where the library removed the pair
    assert cd.tobytes() == np.r_[res["s12"], res["q12"], res["t12"]].tobytes()
