"""Builds tests/initializer_ref.cpp (the CPU restatement of ORB_SLAM2::Initializer) with g++ and loads it with ctypes (test
infrastructure, in the manner of tests/shim_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build
from oracle_lib import KP_DTYPE

_lib = None

RESULT_DTYPE = np.dtype([("initialized", "<i4"), ("model", "<i4"), ("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"),
                         ("best_h", "<i4"), ("best_f", "<i4"), ("H21", "<f4", 9), ("F21", "<f4", 9), ("R21", "<f4", 9),
                         ("t21", "<f4", 3), ("n_good", "<i4"), ("parallax", "<f4")])


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("initializer_ref.cpp")
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        L.ref_initialize.argtypes = [vp, i32, vp, i32, vp, vp, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ref_initialize_use_aruco.argtypes = [vp, i32, vp, i32, vp, vp, f32, vp, i32, vp, vp, vp, vp, vp]
        L.ref_decode_sets.argtypes = [i32, i32, vp, vp]
        L.ref_decode_sets.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _K4(K):
    K = np.asarray(K, np.float32)
    return np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else K.reshape(4), np.float32)


def initialize(kps1, kps2, m12, K, words, sigma=1.0, iterations=200):
    """The restatement's Initialize(): dict with the result record, p3d / triangulated (None when not initialized) and the
    intermediate results (sets, T1, T2, pn1, pn2, H21 / H12 / F21 per hypothesis, SH / SF per hypothesis, sv: the two smallest
    singular values of every eight-point system, H hypotheses then F; for F the second is the residual |A f| of its null vector),
    ninl (inliers of the chosen model) and motion_good (CheckRT's nGood of each motion hypothesis checked)."""
    L = lib()
    k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
    m = np.ascontiguousarray(m12, np.int32); w = np.ascontiguousarray(words, np.int32)
    res = np.zeros(1, RESULT_DTYPE)
    n1, n2 = len(k1), len(k2)
    p3d = np.zeros((max(n1, 1), 3), np.float32); tri = np.zeros(max(n1, 1), np.uint8)
    sets = np.zeros((iterations, 8), np.int32); T = np.zeros(18, np.float32)
    pn1 = np.zeros((max(n1, 1), 2), np.float32); pn2 = np.zeros((max(n2, 1), 2), np.float32)
    models = np.zeros((iterations, 27), np.float32); scores = np.zeros(2 * iterations, np.float32)
    sv = np.zeros((2 * iterations, 2), np.float32)
    mg = np.zeros(10, np.int32)
    N = L.ref_initialize(_p(k1), n1, _p(k2), n2, _p(m), _p(_K4(K)), float(sigma), int(iterations), _p(w), _p(res), _p(p3d), _p(tri),
                         _p(sets), _p(T), _p(pn1), _p(pn2), _p(models), _p(scores), _p(sv), _p(mg))
    r = res[0]
    return dict(N=N, result=r, p3d=p3d[:n1] if r["initialized"] else None, tri=tri[:n1].astype(bool) if r["initialized"] else None,
                sets=sets, T1=T[:9].reshape(3, 3), T2=T[9:].reshape(3, 3), pn1=pn1[:n1], pn2=pn2[:n2],
                H21=models[:, :9].reshape(-1, 3, 3), H12=models[:, 9:18].reshape(-1, 3, 3), F21=models[:, 18:].reshape(-1, 3, 3),
                SH=scores[:iterations], SF=scores[iterations:], sv=sv,
                ninl=int(mg[0]), motion_good=mg[2:2 + mg[1]].copy())


def initialize_use_aruco(kps1, kps2, m12, K, R, t, sigma=1.0):
    L = lib()
    k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
    m = np.ascontiguousarray(m12, np.int32)
    poses = np.ascontiguousarray(np.concatenate([np.asarray(R, np.float32).reshape(-1, 9), np.asarray(t, np.float32).reshape(-1, 3)], 1))
    res = np.zeros(1, RESULT_DTYPE)
    n1 = len(k1)
    p3d = np.zeros((max(n1, 1), 3), np.float32); tri = np.zeros(max(n1, 1), np.uint8)
    ng = np.zeros(max(len(poses), 1), np.int32); par = np.zeros(max(len(poses), 1), np.float32)
    ok = L.ref_initialize_use_aruco(_p(k1), n1, _p(k2), len(k2), _p(m), _p(_K4(K)), float(sigma), _p(poses), len(poses), _p(res),
                                    _p(p3d), _p(tri), _p(ng), _p(par))
    r = res[0]
    have = r["best_h"] >= 0
    return dict(ok=bool(ok), result=r, p3d=p3d[:n1] if have else None, tri=tri[:n1].astype(bool) if have else None,
                n_good=ng[:len(poses)], parallax=par[:len(poses)])


def decode_sets(N, words):
    w = np.ascontiguousarray(words, np.int32)
    out = np.zeros((len(w) // 8, 8), np.int32)
    lib().ref_decode_sets(int(N), len(w) // 8, _p(w), _p(out))
    return out
