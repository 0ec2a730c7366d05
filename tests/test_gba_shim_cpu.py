"""CPU: include/shims/Optimizer_globalba_orbfe.cc compiles -Wall -Werror against the mock trees and links against the library, and its
collect step, run host-only on the hand-built map of tests/gba_shim_map.py, gives the reference's vertices and edge order: bad
keyframes, points and markers skipped, no edge from an observation in a bad keyframe or in one that was not handed over, no marker
without Frame::mbUArucoIni, a stereo observation refused."""
import subprocess

import numpy as np
import pytest

import gba_build
import gba_shim_map as M
from orb_slam2_aruco_amd import binding


@pytest.mark.parametrize("use", [1, 0])
def test_collect_step_gives_the_reference_vertices_and_edge_order(tmp_path, use):
    exe = gba_build.build_shim(str(tmp_path))
    m = M.build()
    pre, post = str(tmp_path / "in"), str(tmp_path / "out")
    M.write(m, pre)
    subprocess.check_call([exe, "collect", pre, post, str(use)])
    pb, vertices, points, markers = M.collect(m, use_markers=bool(use))
    rd = lambda name, t: np.fromfile(post + "_" + name + ".bin", t)
    assert list(rd("vk", np.int32)) == vertices and list(rd("vp", np.int32)) == points and list(rd("vm", np.int32)) == markers
    # the case holds what it says
    kfs, mps = m["kfs"], m["mps"]
    assert len(vertices) == 6 and not any(kfs[k]["bad"] for k in vertices) and m["left_out"] not in vertices and sorted(vertices) != vertices
    assert [kfs[k]["id"] for k in vertices] == sorted(kfs[k]["id"] for k in vertices) and kfs[vertices[0]]["id"] == 0
    assert len(points) == len(mps) - 1 and 17 not in points and markers == ([0, 1] if use else [])
    a = binding.gba_arrays(pb)
    for name, key, t in (("Tcw", "Tcw", np.float32), ("fixed", "kf_fixed", np.uint8), ("x", "x3Dw", np.float32), ("off", "obs_offset", np.int32),
                         ("okf", "obs_kf", np.int32), ("oxy", "obs_xy", np.float32), ("ooct", "obs_octave", np.int32), ("Twm", "Twm", np.float32),
                         ("mloc", "marker_local", np.float32), ("moff", "mobs_offset", np.int32), ("mkf", "mobs_kf", np.int32),
                         ("mcor", "mobs_corners", np.float32), ("K", "K4", np.float32), ("sig", "inv_level_sigma2", np.float32)):
        assert np.array_equal(rd(name, t), a[key].reshape(-1)), name
    assert a["kf_fixed"].tolist() == [1, 0, 0, 0, 0, 0]
    # the observations of a point come in memory order of the keyframes, which is not vertex order; the edgeless point has none
    assert any(list(a["obs_kf"][lo:hi]) != sorted(a["obs_kf"][lo:hi]) for lo, hi in zip(a["obs_offset"][:-1], a["obs_offset"][1:]))
    j = points.index(m["edgeless"])
    assert a["obs_offset"][j + 1] == a["obs_offset"][j] and (np.diff(a["obs_offset"]) == 0).sum() == 1
    # marker 0 is seen from three handed-over keyframes and from the one left out: three observations stay
    assert len(a["mobs_kf"]) == (5 if use else 0)
    assert rd("threw", np.int32)[0] == 1
