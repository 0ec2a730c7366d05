"""GPU: include/shims/Initializer_orbfe.cc, built with g++ against the mock headers of tests/mock_orbslam/, runs one scene the way
Tracking does (Initializer(frame1, 1.0, 200).Initialize(frame2, ...), then InitializeUseAruco) and returns what the C ABI returns for
the same inputs -- the rand() words being those of a fresh process after srand(0), as SeedRandOnce(0) draws them."""
import json
import subprocess
import sys

import numpy as np
import pytest

import shim_build
import initializer_cases as S

pytestmark = pytest.mark.gpu


def _fresh_process_rand(n):
    code = ("import ctypes, json; l = ctypes.CDLL(None); l.srand(0); print(json.dumps([l.rand() for _ in range(%d)]))" % n)
    return np.array(json.loads(subprocess.check_output([sys.executable, "-c", code])), np.int32)


def test_initializer_shim_equals_the_binding(orbfe, tmp_path):
    exe = shim_build.build("init", str(tmp_path))
    sc = S.scene("planar", 800, 0.2, seed=1, noise=0.5)
    tn = sc["t"] / np.linalg.norm(sc["t"])
    R = np.array([np.eye(3), sc["R"], sc["R"].T], np.float32)
    t = np.array([tn, tn, -tn], np.float32)
    K4 = np.array([S.K[0, 0], S.K[1, 1], S.K[0, 2], S.K[1, 2]], np.float32)
    pre = str(tmp_path / "in")
    sc["kps1"].tofile(pre + "_kps1.bin"); sc["kps2"].tofile(pre + "_kps2.bin")
    sc["m12"].astype(np.int32).tofile(pre + "_m12.bin"); K4.tofile(pre + "_K.bin")
    np.concatenate([R.reshape(-1, 9), t], 1).astype(np.float32).tofile(pre + "_poses.bin")
    out = str(tmp_path / "out")
    subprocess.run([exe, pre, out], check=True, timeout=120)
    rd = lambda name, dt: np.fromfile(out + "_" + name + ".bin", dt)

    res, p3d, tri = orbfe.initialize(sc["kps1"], sc["kps2"], sc["m12"], S.K, 1.0, 200, _fresh_process_rand(1600))
    assert res["initialized"] == 1          # the fixture initializes (planar, H branch)
    assert rd("ok", np.int32)[0] == 1
    Rt = rd("Rt", np.float32)
    assert np.array_equal(Rt[:9], res["R21"]) and np.array_equal(Rt[9:], res["t21"])
    assert np.array_equal(rd("p3d", np.float32).reshape(-1, 3), p3d)
    assert np.array_equal(rd("tri", np.uint8).astype(bool), tri)

    ares, ap3d, atri = orbfe.initialize_check_poses(sc["kps1"], sc["kps2"], sc["m12"], S.K, R, t)
    ok, best = rd("aruco", np.int32)
    assert ok == ares["initialized"] and best == ares["best_h"] == 1
    assert np.array_equal(rd("ap3d", np.float32).reshape(-1, 3), ap3d)
    assert np.array_equal(rd("atri", np.uint8).astype(bool), atri)
