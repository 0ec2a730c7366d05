"""Builds tests/pose_opt_ref.cpp (the CPU restatement of ORB_SLAM2's motion-only pose optimization) with g++ and loads it with
ctypes (test infrastructure, in the manner of tests/initializer_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build
from oracle_lib import KP_DTYPE

_lib = None

MARKER_DTYPE = np.dtype([("corners", "<f4", 8), ("Twm", "<f4", 12), ("local", "<f4", 12)])
RESULT_DTYPE = np.dtype([("n_good", "<i4"), ("n_initial", "<i4"), ("n_marker_edges", "<i4"), ("rounds", "<i4"),
                         ("n_bad", "<i4", 4), ("iterations", "<i4", 4), ("stale_mask", "<i4"), ("status", "<i4")])


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("pose_opt_ref.cpp")
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        L.ref_pose_optimization.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, i32, f32, vp, vp, vp, vp, vp]
        L.ref_pose_optimization.restype = i32
        L.ref_marker_jacobian.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.ref_marker_jacobian.restype = None
        L.ref_exp_update.argtypes = [vp, vp, vp]
        L.ref_exp_update.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pose_optimization(pb, outlier_init=None):
    """The restatement on one problem (a dict of tests/pose_opt_cases.py).  Returns dict(rc, Tcw (3 x 4), outlier (uint8, entries
    without a map point keep outlier_init), chi2 (4 x n, NaN where not classified), result record)."""
    L = lib()
    kps = np.ascontiguousarray(pb["kps"], KP_DTYPE)
    n = len(kps)
    has = np.ascontiguousarray(pb["has_mp"], np.uint8)
    X = np.ascontiguousarray(pb["x3Dw"], np.float32).reshape(-1, 3)
    sig = np.ascontiguousarray(pb["inv_sigma2"], np.float32)
    K4 = np.ascontiguousarray(pb["K4"], np.float32)
    mk = np.ascontiguousarray(pb["markers"], MARKER_DTYPE)
    T_in = np.ascontiguousarray(pb["Tcw"], np.float32).reshape(12)
    T_out = np.zeros(12, np.float32)
    out = np.full(max(n, 1), 7 if outlier_init is None else outlier_init, np.uint8)
    chi2 = np.zeros((4, max(n, 1)), np.float64)
    res = np.zeros(1, RESULT_DTYPE)
    rc = L.ref_pose_optimization(_p(kps), n, _p(has), _p(X), _p(sig), len(sig), _p(K4), _p(mk), len(mk), float(pb.get("marker_info", 25.0)),
                                 _p(T_in), _p(T_out), _p(out), _p(chi2), _p(res))
    return dict(rc=rc, Tcw=T_out.reshape(3, 4), outlier=out[:n], chi2=chi2[:, :n], result=res[0])


def marker_jacobian(Tcw, Twm, p, obs, K4):
    J = np.zeros((2, 6)); err = np.zeros(2)
    lib().ref_marker_jacobian(_p(np.ascontiguousarray(Tcw, np.float32).reshape(12)), _p(np.ascontiguousarray(Twm, np.float32).reshape(12)),
                              _p(np.ascontiguousarray(p, np.float64)), _p(np.ascontiguousarray(obs, np.float64)),
                              _p(np.ascontiguousarray(K4, np.float32)), _p(J), _p(err))
    return J, err


def exp_update(u, Tcw):
    out = np.zeros(12, np.float32)
    lib().ref_exp_update(_p(np.ascontiguousarray(u, np.float64)), _p(np.ascontiguousarray(Tcw, np.float32).reshape(12)), _p(out))
    return out.reshape(3, 4)
