"""GPU: include/shims/Sim3Solver_orbfe.cc, built with g++ against the mock headers of tests/mock_orbslam/, runs three solvers the way
LoopClosing::ComputeSim3 does (SetRansacParameters(0.99, 20, 300), then iterate(5) on each candidate in turn until none has more) and
returns, call for call, what the C ABI returns for the same inputs through binding.Sim3Solver -- fed the rand() words the shim drew
(the driver supplies rand() itself and dumps every value, tests/sim3_shim_driver.cpp), in the shim's own schedule of
3 * min(5, remaining) words a call."""
import subprocess

import numpy as np
import pytest

import sim3_build as B
import sim3_cases as S
import shim_build

pytestmark = pytest.mark.gpu
SEED = 4242


def test_sim3_shim_equals_the_binding_over_interleaved_solvers(orbfe, tmp_path):
    exe = shim_build.build("sim3", str(tmp_path))
    # a candidate that succeeds late, one that never has enough correspondences, one that succeeds at once
    scenes = [S.scene(100, 1.3, 0.6, False, seed=4), S.scene(19, 1.0, 0.0, True, seed=4), S.scene(40, 0.7, 0.3, False, seed=4)]
    pre = str(tmp_path / "in")
    for j, sc in enumerate(scenes):
        p = "%s_%d_" % (pre, j)
        sc["kps1"].tofile(p + "kps1.bin"); sc["kps2"].tofile(p + "kps2.bin")
        sc["x3Dw1"].tofile(p + "x1.bin"); sc["x3Dw2"].tofile(p + "x2.bin")
        sc["valid1"].tofile(p + "v1.bin"); sc["valid2"].tofile(p + "v2.bin")
        sc["m12"].astype(np.int32).tofile(p + "m12.bin")
        sc["Tcw1"].tofile(p + "T1.bin"); sc["Tcw2"].tofile(p + "T2.bin")
        sc["K4_1"].tofile(p + "K.bin"); sc["level_sigma2"].tofile(p + "ls2.bin")
        np.array([int(sc["fix_scale"])], np.int32).tofile(p + "fix.bin")
    out = str(tmp_path / "out")
    subprocess.run([exe, pre, out, str(len(scenes)), str(SEED)], check=True, timeout=180)
    ci = np.fromfile(out + "_i.bin", np.int32).reshape(-1, 5)
    cf = np.fromfile(out + "_f.bin", np.float32).reshape(-1, 29)
    cinl = np.fromfile(out + "_inl.bin", np.uint8)

    sols, max_its = [], []
    for sc in scenes:
        s = orbfe.Sim3Solver((sc["kps1"], sc["x3Dw1"], sc["valid1"], sc["Tcw1"], sc["K4_1"]),
                             (sc["kps2"], sc["x3Dw2"], sc["valid2"], sc["Tcw2"], sc["K4_2"]), sc["m12"], sc["level_sigma2"], sc["fix_scale"])
        s.set_ransac_parameters(*S.RANSAC)
        sols.append(s)
        max_its.append(int(B.solve(sc, *S.RANSAC, words=S.words(300, 0))["result"]["max_iterations"]))
    stream = np.fromfile(out + "_words.bin", np.int32)
    assert stream.min() >= 0
    drawn, off, found_any = 0, 0, 0
    done = [False] * len(scenes)
    for call, (j, has, no_more, n_inl, n1) in enumerate(ci.tolist()):
        sc, s = scenes[j], sols[j]
        assert not done[j] and n1 == len(sc["kps1"])
        N = int(np.count_nonzero((sc["m12"] >= 0) & (sc["valid1"] != 0) & (sc["valid2"][np.maximum(sc["m12"], 0)] != 0)))
        flags = cinl[off:off + n1].astype(bool); off += n1
        n = min(5, max_its[j] - s.iterations)
        if N < S.RANSAC[1] or n <= 0:
            # the shim answers these without a library call and without drawing
            assert not has and no_more and n_inl == 0 and not flags.any()
            done[j] = True
            continue
        w = stream[drawn:drawn + 3 * n]; drawn += 3 * n
        assert len(w) == 3 * n, (call, j)
        T, g_no_more, g_flags, g_n = s.iterate(n, w)
        assert has == (T is not None) and bool(no_more) == g_no_more and n_inl == g_n, (call, j)
        assert np.array_equal(flags, g_flags), (call, j)
        if T is not None:
            found_any += 1
            assert np.array_equal(cf[call, :16].view(np.uint32), T.ravel().view(np.uint32)), (call, j)
            assert np.array_equal(cf[call, 16:25].view(np.uint32), s.R12.ravel().view(np.uint32))
            assert np.array_equal(cf[call, 25:28].view(np.uint32), s.t12.view(np.uint32))
            assert cf[call, 28:29].view(np.uint32)[0] == np.float32(s.s12).view(np.uint32)
        else:
            assert not cf[call].any()
        done[j] = bool(no_more)
    assert off == len(cinl) and all(done) and found_any >= 2
    assert drawn == len(stream)      # the shim drew exactly the windows' words
    print("shim: %d calls over %d solvers, %d returned a transform, %d words drawn" % (len(ci), len(scenes), found_any, drawn))
