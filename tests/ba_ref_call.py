"""The ctypes calls the two bundle adjustment restatements share (test infrastructure; tests/lba_build.py and tests/gba_build.py load
tests/lba_ref.cpp and tests/gba_ref.cpp, which both include tests/ba_ref.hpp): the pointer helpers, the flat problem as the struct
Flat of tests/ba_ref.hpp, the two single-edge wrappers, and the unpacking of an inspect call."""
import ctypes as C

import numpy as np

INSERTION, DEVICE = 0, 1     # the summation orders of the restatements
vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float


class Flat(C.Structure):
    """struct Flat of tests/ba_ref.hpp: the problem arguments of include/orbfe.h's two bundle adjustments, in their order"""
    _fields_ = [("Tcw", vp), ("kf_fixed", vp), ("nkf", i32), ("x3Dw", vp), ("np", i32), ("obs_offset", vp), ("obs_kf", vp), ("obs_xy", vp),
                ("obs_octave", vp), ("nobs", i32), ("K4", vp), ("inv_sigma2", vp), ("nlevels", i32), ("Twm", vp), ("marker_local", vp),
                ("nma", i32), ("mobs_offset", vp), ("mobs_kf", vp), ("mobs_corners", vp), ("nmobs", i32), ("marker_info", f32),
                ("use_markers", i32)]


def declare(lib, calls):
    """argtypes for the calls of a restatement that take the problem first ({name: the types after it}), and for the two edge calls"""
    for name, rest in calls.items():
        getattr(lib, name).argtypes = [C.POINTER(Flat)] + rest
        getattr(lib, name).restype = C.c_int
    for name in ("ref_ba_mono_edge", "ref_ba_marker_edge"):
        getattr(lib, name).argtypes = [vp] * 8
        getattr(lib, name).restype = None
    return lib


def p(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(vp)


def problem(a):
    """the arrays of binding.lba_arrays / binding.gba_arrays as a Flat; `a` keeps them alive"""
    return C.byref(Flat(p(a["Tcw"]), p(a["kf_fixed"]), len(a["Tcw"]), p(a["x3Dw"]), len(a["x3Dw"]), p(a["obs_offset"]), p(a["obs_kf"]), p(a["obs_xy"]),
                        p(a["obs_octave"]), len(a["obs_kf"]), p(a["K4"]), p(a["inv_level_sigma2"]), len(a["inv_level_sigma2"]), p(a["Twm"]),
                        p(a["marker_local"]), len(a["Twm"]), p(a["mobs_offset"]), p(a["mobs_kf"]), p(a["mobs_corners"]), len(a["mobs_kf"]),
                        a["marker_info"], a["use_markers"]))


def inspect_buffers(n, V, nchi2, full, pad=0):
    """nv, b, Hpp, Hll, chi2, x and H (None unless full) of an inspect call with n points and at most V pose vertices"""
    b = np.zeros(6 * V + 3 * n + pad)
    return dict(nv=np.zeros(1, np.int32), b=b, Hpp=np.zeros((max(V, 1), 6, 6)), Hll=np.zeros((max(n, 1), 6)), chi2=np.zeros(nchi2), x=np.zeros_like(b),
                H=np.zeros((6 * V + 3 * n) ** 2 + pad) if full else None)


def inspect_unpack(w, n, full):
    """the dict binding.lba_inspect / gba_inspect return, from the filled buffers; full adds H, b and x of the whole system"""
    v, b, x = int(w["nv"][0]), w["b"], w["x"]
    out = dict(nv=v, b_pose=b[:6 * v].reshape(v, 6), b_point=b[6 * v:6 * v + 3 * n].reshape(n, 3), Hpp=w["Hpp"][:v], Hll=w["Hll"][:n], chi2=w["chi2"][0],
               lambda0=w["chi2"][1], x_pose=x[:6 * v].reshape(v, 6), x_point=x[6 * v:6 * v + 3 * n].reshape(n, 3))
    if full:
        m = 6 * v + 3 * n
        out["H"] = w["H"][:m * m].reshape(m, m)
        out["b"] = b[:m].copy()
        out["x"] = x[:m].copy()
    return out


def _d(a):
    return np.ascontiguousarray(a, np.float64)


def _f(a, n):
    return np.ascontiguousarray(a, np.float32).reshape(n)


def mono_edge(lib, Tcw, u, X, obs, K4):
    """(err, Jpose 2 x 6, Jpoint 2 x 3) of one EdgeSE3ProjectXYZ at exp(u) * Tcw and X."""
    err = np.zeros(2); Jp = np.zeros((2, 6)); Jx = np.zeros((2, 3))
    u, X, obs, T, K = _d(u), _d(X), _d(obs), _f(Tcw, 12), _f(K4, 4)
    lib.ref_ba_mono_edge(p(T), p(u), p(X), p(obs), p(K), p(err), p(Jp), p(Jx))
    return err, Jp, Jx


def marker_edge(lib, Tcw, Twm, pm, obs, K4):
    """(err, Jcamera 2 x 6, Jmarker 2 x 6): one EdgeMarker with g2o's numeric Jacobians."""
    err = np.zeros(2); Jc = np.zeros((2, 6)); Jm = np.zeros((2, 6))
    Tc, Tm, pm, obs, K = _f(Tcw, 12), _f(Twm, 12), _d(pm), _d(obs), _f(K4, 4)
    lib.ref_ba_marker_edge(p(Tc), p(Tm), p(pm), p(obs), p(K), p(err), p(Jc), p(Jm))
    return err, Jc, Jm
