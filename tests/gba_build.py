"""Builds tests/gba_ref.cpp (the CPU restatement of ORB_SLAM2's Optimizer::BundleAdjustment) with g++ and loads it with ctypes
(test infrastructure, in the manner of tests/lba_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build
from orb_slam2_aruco_amd import binding

_lib = None

RESULT_DTYPE = binding.GBA_RESULT_DTYPE
INSERTION, DEVICE = 0, 1     # the summation orders of the restatement


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("gba_ref.cpp")
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        prob = [vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, f32, i32]
        L.ref_gba.argtypes = prob + [i32, i32, i32, vp, vp]
        L.ref_gba.restype = i32
        L.ref_gba_inspect.argtypes = prob + [i32, i32] + [vp] * 8
        L.ref_gba_inspect.restype = i32
        L.ref_gba_mono_edge.argtypes = [vp] * 8
        L.ref_gba_mono_edge.restype = None
        L.ref_gba_marker_edge.argtypes = [vp] * 8
        L.ref_gba_marker_edge.restype = None
        _lib = L
    return _lib


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


def _args(a):
    return [_p(a["Tcw"]), _p(a["kf_fixed"]), len(a["Tcw"]), _p(a["x3Dw"]), len(a["x3Dw"]), _p(a["obs_offset"]), _p(a["obs_kf"]), _p(a["obs_xy"]),
            _p(a["obs_octave"]), len(a["obs_kf"]), _p(a["K4"]), _p(a["inv_level_sigma2"]), len(a["inv_level_sigma2"]), _p(a["Twm"]),
            _p(a["marker_local"]), len(a["Twm"]), _p(a["mobs_offset"]), _p(a["mobs_kf"]), _p(a["mobs_corners"]), len(a["mobs_kf"]),
            a["marker_info"], a["use_markers"]]


def global_bundle_adjustment(pb, order=INSERTION, iterations=None):
    """The restatement on one problem (a dict of tests/gba_cases.py).  Returns what binding.global_bundle_adjustment returns, and
    err: the error of every edge (monocular, then marker corners; pixels) at the final estimates in double, before they are rounded
    to float.  iterations: instead of the problem's own, and not bounded by the library's 20."""
    a = binding.gba_arrays(pb)
    res = np.zeros(1, RESULT_DTYPE)
    err = np.zeros((len(a["obs_kf"]) + (4 * len(a["mobs_kf"]) if a["use_markers"] else 0) + 1, 2))
    rc = lib().ref_gba(*(_args(a) + [a["iterations"] if iterations is None else int(iterations), a["robust"], int(order), _p(res), _p(err)]))
    assert rc == 0, rc
    return dict(Tcw=a["Tcw"].reshape(-1, 3, 4), x3Dw=a["x3Dw"], Twm=a["Twm"].reshape(-1, 3, 4), result=res[0], err=err[:-1])


def inspect(pb, order=DEVICE, full=False, reduced=False):
    """As binding.gba_inspect without the tree; full=True adds H (the whole system with lambda0 on its diagonal, poses first), b (its
    right side) and x; reduced=True adds S (the dense reduced system at lambda0)."""
    a = binding.gba_arrays(pb)
    n, V = len(a["x3Dw"]), len(a["Tcw"]) + len(a["Twm"])
    nv = np.zeros(1, np.int32)
    b = np.zeros(6 * V + 3 * n + 1); x = np.zeros_like(b)
    Hpp = np.zeros((max(V, 1), 6, 6)); Hll = np.zeros((max(n, 1), 6)); chi2 = np.zeros(3)
    H = np.zeros((6 * V + 3 * n) ** 2 + 1) if full else None
    S = np.zeros((6 * V) ** 2 + 1) if reduced else None
    rc = lib().ref_gba_inspect(*(_args(a) + [a["robust"], int(order), _p(nv), _p(b), _p(Hpp), _p(Hll), _p(chi2), _p(x), _p(H), _p(S)]))
    assert rc == 0, rc
    v = int(nv[0])
    out = dict(nv=v, b_pose=b[:6 * v].reshape(v, 6), b_point=b[6 * v:6 * v + 3 * n].reshape(n, 3), Hpp=Hpp[:v], Hll=Hll[:n], chi2=chi2[0],
               lambda0=chi2[1], solved=bool(chi2[2]), x_pose=x[:6 * v].reshape(v, 6), x_point=x[6 * v:6 * v + 3 * n].reshape(n, 3))
    m = 6 * v + 3 * n
    if full:
        out["H"] = H[:m * m].reshape(m, m)
        out["b"] = b[:m].copy()
        out["x"] = x[:m].copy()
    if reduced:
        out["S"] = S[:36 * v * v].reshape(6 * v, 6 * v)
    return out


def _d(a):
    return np.ascontiguousarray(a, np.float64)


def _f(a, n):
    return np.ascontiguousarray(a, np.float32).reshape(n)


def mono_edge(Tcw, u, X, obs, K4):
    """(err, Jpose 2 x 6, Jpoint 2 x 3) of one EdgeSE3ProjectXYZ at exp(u) * Tcw and X."""
    err = np.zeros(2); Jp = np.zeros((2, 6)); Jx = np.zeros((2, 3))
    u, X, obs, T, K = _d(u), _d(X), _d(obs), _f(Tcw, 12), _f(K4, 4)
    lib().ref_gba_mono_edge(_p(T), _p(u), _p(X), _p(obs), _p(K), _p(err), _p(Jp), _p(Jx))
    return err, Jp, Jx


def marker_edge(Tcw, Twm, p, obs, K4):
    """(err, Jcamera 2 x 6, Jmarker 2 x 6): one EdgeMarker with g2o's numeric Jacobians."""
    err = np.zeros(2); Jc = np.zeros((2, 6)); Jm = np.zeros((2, 6))
    Tc, Tm, p, obs, K = _f(Tcw, 12), _f(Twm, 12), _d(p), _d(obs), _f(K4, 4)
    lib().ref_gba_marker_edge(_p(Tc), _p(Tm), _p(p), _p(obs), _p(K), _p(err), _p(Jc), _p(Jm))
    return err, Jc, Jm


def build_shim(out_dir):
    """include/shims/Optimizer_globalba_orbfe.cc and tests/gba_shim_driver.cpp as one program: the fuller mock headers of
    tests/mock_orbslam_gba/ ahead of tests/mock_orbslam_lba/ and the one mock tree tests/mock_orbslam/, linked against the built library."""
    import os
    import subprocess
    root, here = ref_build.ROOT, ref_build.HERE
    inc = []
    for d in ("tests/mock_orbslam_gba", "tests/mock_orbslam_lba") + ref_build.MOCK_DIRS + ("include", "include/shims", "tests"):
        inc += ["-I", os.path.join(root, d)]
    flags = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-pthread"]
    objs = []
    for src in (os.path.join(root, "include", "shims", "Optimizer_globalba_orbfe.cc"), os.path.join(here, "mock_orbslam", "Frame_statics.cc")):
        objs.append(os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0] + ".o"))
        subprocess.check_call(flags + inc + ["-c", src, "-o", objs[-1]])
    exe = os.path.join(out_dir, "gba_shim_driver")
    lib_dir = os.path.join(root, "orb_slam2_aruco_amd")
    subprocess.check_call(flags + inc + [os.path.join(here, "gba_shim_driver.cpp")] + objs + ["-o", exe, "-L", lib_dir, "-lorbfe", "-Wl,-rpath," + lib_dir])
    return exe
