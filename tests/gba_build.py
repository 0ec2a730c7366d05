"""Builds tests/gba_ref.cpp (the CPU restatement of ORB_SLAM2's Optimizer::BundleAdjustment) with g++ and loads it with ctypes
(test infrastructure, in the manner of tests/lba_build.py).  One build per process, in a temporary directory.  What it shares with
tests/lba_build.py is in tests/ba_ref_call.py."""
import functools

import numpy as np

import ba_ref_call as R
import ref_build
from ba_ref_call import INSERTION, DEVICE   # noqa: F401
from orb_slam2_aruco_amd import binding

RESULT_DTYPE = binding.GBA_RESULT_DTYPE
_p = R.p


@functools.lru_cache(None)
def lib():
    return R.declare(ref_build.build_shared("gba_ref.cpp"), dict(ref_gba=[R.i32] * 3 + [R.vp] * 2, ref_gba_inspect=[R.i32] * 2 + [R.vp] * 8))


def global_bundle_adjustment(pb, order=INSERTION, iterations=None):
    """The restatement on one problem (a dict of tests/gba_cases.py).  Returns what binding.global_bundle_adjustment returns, and
    err: the error of every edge (monocular, then marker corners; pixels) at the final estimates in double, before they are rounded
    to float.  iterations: instead of the problem's own, and not bounded by the library's 20."""
    a = binding.gba_arrays(pb)
    res = np.zeros(1, RESULT_DTYPE)
    err = np.zeros((len(a["obs_kf"]) + (4 * len(a["mobs_kf"]) if a["use_markers"] else 0) + 1, 2))
    rc = lib().ref_gba(R.problem(a), a["iterations"] if iterations is None else int(iterations), a["robust"], int(order), _p(res), _p(err))
    assert rc == 0, rc
    return dict(Tcw=a["Tcw"].reshape(-1, 3, 4), x3Dw=a["x3Dw"], Twm=a["Twm"].reshape(-1, 3, 4), result=res[0], err=err[:-1])


def inspect(pb, order=DEVICE, full=False, reduced=False):
    """As binding.gba_inspect without the tree; full=True adds H (the whole system with lambda0 on its diagonal, poses first), b (its
    right side) and x; reduced=True adds S (the dense reduced system at lambda0)."""
    a = binding.gba_arrays(pb)
    n, V = len(a["x3Dw"]), len(a["Tcw"]) + len(a["Twm"])
    w = R.inspect_buffers(n, V, 3, full, pad=1)
    S = np.zeros((6 * V) ** 2 + 1) if reduced else None
    rc = lib().ref_gba_inspect(R.problem(a), a["robust"], int(order), *[_p(w[k]) for k in ("nv", "b", "Hpp", "Hll", "chi2", "x", "H")], _p(S))
    assert rc == 0, rc
    out = dict(R.inspect_unpack(w, n, full), solved=bool(w["chi2"][2]))
    if reduced:
        out["S"] = S[:36 * out["nv"] ** 2].reshape(6 * out["nv"], 6 * out["nv"])
    return out


def mono_edge(Tcw, u, X, obs, K4):
    return R.mono_edge(lib(), Tcw, u, X, obs, K4)


def marker_edge(Tcw, Twm, p, obs, K4):
    return R.marker_edge(lib(), Tcw, Twm, p, obs, K4)


def build_shim(out_dir):
    """include/shims/Optimizer_globalba_orbfe.cc and tests/gba_shim_driver.cpp as one program"""
    return ref_build.build_shim(("Optimizer_globalba_orbfe.cc",), "gba_shim_driver.cpp", out_dir)
