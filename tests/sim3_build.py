"""Builds tests/sim3_ref.cpp (the CPU restatement of ORB_SLAM2::Sim3Solver) with g++ and loads it with ctypes (test infrastructure,
in the manner of tests/initializer_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build
from oracle_lib import KP_DTYPE

_lib = None

RESULT_DTYPE = np.dtype([("n", "<i4"), ("max_iterations", "<i4"), ("no_more", "<i4"), ("found", "<i4"), ("n_inliers", "<i4"),
                         ("best", "<i4"), ("best_inliers", "<i4"), ("s12", "<f4"), ("R12", "<f4", 9), ("t12", "<f4", 3),
                         ("T12", "<f4", 16), ("status", "<i4")])


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("sim3_ref.cpp")
        vp, i32 = C.c_void_p, C.c_int
        side = [vp, i32, vp, vp, vp, vp]
        L.ref_sim3.argtypes = side + side + [vp, vp, i32, i32, C.c_double, i32, i32, i32, i32, i32, vp] + [vp] * 13
        L.ref_sim3_decode_sets.argtypes = [i32, i32, vp, vp]
        L.ref_sim3_decode_sets.restype = None
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def solve(sc, probability=0.99, min_inliers=20, max_iterations=300, first=0, n_iterations=None, best_in=0, words=None):
    """One iterate() window of the restatement on a scene of sim3_cases.scene(): dict with the result record, inliers12, N, indices1,
    X3Dc1 / X3Dc2, P1im1 / P2im2, maxError1 / 2, and per hypothesis of the window sets, s12, R12, t12, counts and eig (the two
    largest eigenvalues of N).  Raises ValueError for an octave outside the level table."""
    L = lib()
    n_iterations = max_iterations if n_iterations is None else n_iterations
    k1 = np.ascontiguousarray(sc["kps1"], KP_DTYPE); k2 = np.ascontiguousarray(sc["kps2"], KP_DTYPE)
    x1 = np.ascontiguousarray(sc["x3Dw1"], np.float32); x2 = np.ascontiguousarray(sc["x3Dw2"], np.float32)
    v1 = None if sc.get("valid1") is None else np.ascontiguousarray(sc["valid1"], np.uint8)
    v2 = None if sc.get("valid2") is None else np.ascontiguousarray(sc["valid2"], np.uint8)
    T1 = np.ascontiguousarray(sc["Tcw1"], np.float32); T2 = np.ascontiguousarray(sc["Tcw2"], np.float32)
    K1 = np.ascontiguousarray(sc["K4_1"], np.float32); K2 = np.ascontiguousarray(sc["K4_2"], np.float32)
    m = np.ascontiguousarray(sc["m12"], np.int32); ls2 = np.ascontiguousarray(sc["level_sigma2"], np.float32)
    w = np.ascontiguousarray(words, np.int32)
    assert len(w) >= 3 * n_iterations
    n1, it = max(len(k1), 1), n_iterations
    res = np.zeros(1, RESULT_DTYPE); inl = np.zeros(n1, np.uint8)
    idx = np.zeros(n1, np.int32); X1 = np.zeros((n1, 3), np.float32); X2 = np.zeros((n1, 3), np.float32)
    P1 = np.zeros((n1, 2), np.float32); P2 = np.zeros((n1, 2), np.float32); e1 = np.zeros(n1, np.float32); e2 = np.zeros(n1, np.float32)
    sets = np.zeros((it, 3), np.int32); models = np.zeros((it, 13), np.float32); counts = np.zeros(it, np.int32)
    eig = np.zeros((it, 2), np.float32)
    N = L.ref_sim3(_p(k1), len(k1), _p(x1), _p(v1), _p(T1), _p(K1), _p(k2), len(k2), _p(x2), _p(v2), _p(T2), _p(K2), _p(m), _p(ls2),
                   len(ls2), int(bool(sc["fix_scale"])), float(probability), int(min_inliers), int(max_iterations), int(first), int(it),
                   int(best_in), _p(w), _p(res), _p(inl), _p(idx), _p(X1), _p(X2), _p(P1), _p(P2), _p(e1), _p(e2), _p(sets), _p(models),
                   _p(counts), _p(eig))
    if N < 0:
        raise ValueError("octave outside the level table")
    return dict(result=res[0], inliers12=inl[:len(k1)].astype(bool), N=N, indices1=idx[:N], X3Dc1=X1[:N], X3Dc2=X2[:N], P1im1=P1[:N],
                P2im2=P2[:N], maxError1=e1[:N], maxError2=e2[:N], sets=sets, s12=models[:, 0], R12=models[:, 1:10].reshape(-1, 3, 3),
                t12=models[:, 10:13], counts=counts, eig=eig)


def decode_sets(N, words):
    w = np.ascontiguousarray(words, np.int32)
    out = np.zeros((len(w) // 3, 3), np.int32)
    lib().ref_sim3_decode_sets(int(N), len(w) // 3, _p(w), _p(out))
    return out
