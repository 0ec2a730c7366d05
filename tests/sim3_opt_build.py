"""Builds tests/sim3_opt_ref.cpp (the CPU restatement of ORB_SLAM2's Optimizer::OptimizeSim3) with g++ and loads it with ctypes
(test infrastructure, in the manner of tests/pose_opt_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build
from oracle_lib import KP_DTYPE

_lib = None

RESULT_DTYPE = np.dtype([("n_inliers", "<i4"), ("n_correspondences", "<i4"), ("n_bad", "<i4"), ("more_iterations", "<i4"),
                         ("iterations", "<i4", 2), ("stale_mask", "<i4"), ("status", "<i4"), ("s12", "<f8"), ("q12", "<f8", 4),
                         ("t12", "<f8", 3)])
INSERTION, DEVICE = 0, 1     # the summation orders of the restatement


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("sim3_opt_ref.cpp")
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        side = [vp, i32, vp, vp, vp, vp]
        L.ref_optimize_sim3.argtypes = side + side + [vp, vp, i32, f32, vp, vp, f32, i32, i32, vp, vp, vp]
        L.ref_optimize_sim3.restype = i32
        L.ref_sim3_edge_jacobians.argtypes = [f32, vp, vp, i32] + [vp] * 10
        L.ref_sim3_edge_jacobians.restype = None
        L.ref_sim3_oplus.argtypes = [vp, f32, vp, vp, i32, vp]
        L.ref_sim3_oplus.restype = None
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, n):
    return np.ascontiguousarray(a, np.float32).reshape(n)


def optimize_sim3(pb, order=INSERTION):
    """The restatement on one problem (a dict of tests/sim3_opt_cases.py).  Returns dict(rc, match12 (n1 ints), chi2 (2 checks x n1 x
    2: e12 and e21 of every pair a check looked at, NaN elsewhere), result record)."""
    L = lib()
    k1 = np.ascontiguousarray(pb["kps1"], KP_DTYPE); k2 = np.ascontiguousarray(pb["kps2"], KP_DTYPE)
    n1, n2 = len(k1), len(k2)
    x1 = _f32(pb["x3Dw1"], (-1, 3)); x2 = _f32(pb["x3Dw2"], (-1, 3))
    v1 = None if pb["valid1"] is None else np.ascontiguousarray(pb["valid1"], np.uint8)
    v2 = None if pb["valid2"] is None else np.ascontiguousarray(pb["valid2"], np.uint8)
    m12 = np.ascontiguousarray(pb["m12"], np.int32)
    sig = _f32(pb["inv_sigma2"], -1)
    out = np.full(max(n1, 1), -7, np.int32)
    chi2 = np.full((2, max(n1, 1), 2), np.nan)
    res = np.zeros(1, RESULT_DTYPE)
    rc = L.ref_optimize_sim3(_p(k1), n1, _p(x1), _p(v1), _p(_f32(pb["Tcw1"], 12)), _p(_f32(pb["K4_1"], 4)),
                             _p(k2), n2, _p(x2), _p(v2), _p(_f32(pb["Tcw2"], 12)), _p(_f32(pb["K4_2"], 4)),
                             _p(m12), _p(sig), len(sig), float(pb["s12_0"]), _p(_f32(pb["R12_0"], 9)), _p(_f32(pb["t12_0"], 3)),
                             float(pb["th2"]), int(pb["fix_scale"]), int(order), _p(out), _p(res), _p(chi2))
    return dict(rc=rc, match12=out[:n1], chi2=chi2[:, :n1], result=res[0])


def edge_jacobians(s12, R12, t12, fix_scale, P1, P2, obs1, obs2, K4_1, K4_2):
    """(J12 2 x 7, J21 2 x 7, err12, err21): the numeric Jacobians and errors of the two edge types at one correspondence."""
    J12 = np.zeros((2, 7)); J21 = np.zeros((2, 7)); e12 = np.zeros(2); e21 = np.zeros(2)
    d = lambda a: np.ascontiguousarray(a, np.float64)
    lib().ref_sim3_edge_jacobians(float(s12), _p(_f32(R12, 9)), _p(_f32(t12, 3)), int(fix_scale), _p(d(P1)), _p(d(P2)), _p(d(obs1)),
                                  _p(d(obs2)), _p(_f32(K4_1, 4)), _p(_f32(K4_2, 4)), _p(J12), _p(J21), _p(e12), _p(e21))
    return J12, J21, e12, e21


def oplus(u, s12, R12, t12, fix_scale):
    """Sim3(update) * S as (s, q (x, y, z, w), t)."""
    out = np.zeros(8)
    lib().ref_sim3_oplus(_p(np.ascontiguousarray(u, np.float64)), float(s12), _p(_f32(R12, 9)), _p(_f32(t12, 3)), int(fix_scale), _p(out))
    return out[0], out[1:5].copy(), out[5:8].copy()
