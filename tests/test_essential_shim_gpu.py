"""GPU test of include/shims/Optimizer_essential_orbfe.cc: Optimizer::OptimizeEssentialGraph on the mock map of
tests/essential_shim_driver.cpp against the binding on the arrays the shim collected, bit for bit, and the apply step's bookkeeping."""
import numpy as np
import pytest

import essential_shim_build as B

pytestmark = pytest.mark.gpu


def test_shim_on_the_mock_map_equals_the_binding(orbfe, tmp_path):
    out = str(tmp_path)
    d = B.run(B.build_driver(out), "run", out)
    pb = B.problem(d)
    want = orbfe.optimize_essential_graph(pb)
    assert want["result"]["iterations"] > 0 and want["result"]["chi2_last"] < want["result"]["chi2_first"]
    T = d["T"].reshape(8, 3, 4)
    vk = d["vk"].tolist()
    assert np.array_equal(T[vk].view(np.uint32), want["Tcw"].view(np.uint32))
    counts = d["counts"]
    assert counts[:8].tolist() == [1, 1, 1, 1, 1, 0, 1, 1]          # SetPose once per vertex, never for the bad keyframe
    assert not np.array_equal(T[7], pb["Tcw"][6]) and np.allclose(T[1], pb["Tcw"][1], atol=1e-6)   # the loop keyframe stays
    P = d["P"].reshape(12, 3)
    pc = counts[8:32].reshape(12, 2)
    moved = [i for i in range(12) if i not in (6, 8)]
    assert np.array_equal(P[moved].view(np.uint32), want["x3Dw"][moved].view(np.uint32))
    assert np.array_equal(P[[6, 8, 11]], pb["x3Dw"][[6, 8, 11]])    # bad; the skipped marker point; the point of a bad keyframe
    assert pc[:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1] and pc[:, 1].tolist() == pc[:, 0].tolist()
    assert not np.array_equal(P[7], pb["x3Dw"][7])                  # corrected through keyframe 6, which moved
    # the marker of keyframe 3: updated once, with the corrected pose's Rwc and centre
    assert counts[32:].tolist() == [1, 1, 0, 3]
    R, t = T[3][:, :3], T[3][:, 3]
    assert np.array_equal(d["M"][:9].reshape(3, 3), R.T)
    assert np.allclose(d["M"][9:], -R.T @ t, atol=1e-6)
