"""CPU: include/shims/Optimizer_localba_orbfe.cc compiles -Wall -Werror against the mock trees and links against the library, and
its collect step, run host-only on the hand-built map of tests/lba_shim_map.py, gives the reference's lists (local and fixed
keyframes, local points, markers), marks, and edge order."""
import subprocess

import numpy as np

import lba_build
import lba_shim_map as M
from orb_slam2_aruco_amd import binding


def test_collect_step_gives_the_reference_lists_and_edge_order(tmp_path):
    exe = lba_build.build_shim(str(tmp_path))
    m = M.build()
    pre, post = str(tmp_path / "in"), str(tmp_path / "out")
    M.write(m, pre)
    subprocess.check_call([exe, "collect", pre, post])
    pb, vertices, nlocal, points, markers, edges = M.collect(m)
    rd = lambda name, t: np.fromfile(post + "_" + name + ".bin", t)
    vk = rd("vk", np.int32)
    assert list(vk[:-1]) == vertices and vk[-1] == nlocal
    assert list(rd("vp", np.int32)) == points and list(rd("vm", np.int32)) == markers
    # the case holds what it says: a fixed camera, a bad covisible keyframe and a non-vertex keyframe left out, the mnId 0 keyframe local
    kfs = m["kfs"]
    assert nlocal == 4 and len(vertices) == 6 and not any(kfs[k]["bad"] for k in vertices) and len(markers) == 2 and 80 <= len(points) < 90 and 17 not in points
    assert sorted(vertices) != vertices and any(kfs[k]["id"] == 0 for k in vertices[:nlocal])
    marks = rd("marks", np.int32).reshape(-1, 2)
    cur_id = kfs[m["cur"]]["id"]
    assert [i for i in range(len(kfs)) if marks[i, 0] == cur_id] == sorted([m["cur"]] + m["cov"])
    assert [i for i in range(len(kfs)) if marks[i, 1] == cur_id] == sorted(vertices[nlocal:])
    a = binding.lba_arrays(pb)
    for name, key, t in (("Tcw", "Tcw", np.float32), ("fixed", "kf_fixed", np.uint8), ("x", "x3Dw", np.float32), ("off", "obs_offset", np.int32),
                         ("okf", "obs_kf", np.int32), ("oxy", "obs_xy", np.float32), ("ooct", "obs_octave", np.int32), ("Twm", "Twm", np.float32),
                         ("mloc", "marker_local", np.float32), ("moff", "mobs_offset", np.int32), ("mkf", "mobs_kf", np.int32),
                         ("mcor", "mobs_corners", np.float32), ("K", "K4", np.float32), ("sig", "inv_level_sigma2", np.float32)):
        assert np.array_equal(rd(name, t), a[key].reshape(-1)), name
    # the observations of a point come in memory order of the keyframes, which is not vertex order
    assert any(list(a["obs_kf"][lo:hi]) != sorted(a["obs_kf"][lo:hi]) for lo, hi in zip(a["obs_offset"][:-1], a["obs_offset"][1:]))
    assert len(a["mobs_kf"]) == 5 and a["kf_fixed"].sum() == 3
    assert rd("threw", np.int32)[0] == 1
