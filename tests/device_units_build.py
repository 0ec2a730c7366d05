"""Builds the unit probe of the shared device helpers (test infrastructure, in the manner of tests/blur_layout_build.py).

probe()             tests/device_units_probe.hip, compiled once per process into a temporary directory with hipcc and exactly the flags
                    build() gives the library's sources (__graft_entry__.HIPCC_FLAGS + ORBFE_EXTRA_HIPCC_FLAGS), loaded with ctypes.
                    The probe includes include/orbfe_math.h and csrc/{wave_dpp,lm_dense,ransac_sets,sim3_points,aruco_pose}.hpp unchanged; it is
                    not part of liborbfe.so.
host()              tests/device_units_host.cpp (include/orbfe_math.h under g++ -ffp-contract=off), the same array calls for the math group.
sanitizer_program() that host file as a program of its own under -fsanitize=address,undefined; returns its path.

The wrappers below take and return numpy arrays; `L` is probe() or host() for the math group, probe() for the rest.  A HIP error code
other than 0 raises."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import ref_build

import __graft_entry__ as entry

_probe = None
_host = None
SOURCE = os.path.join(ref_build.HERE, "device_units_probe.hip")
vp, i32 = C.c_void_p, C.c_int
_MATH = {"du_atan2": [vp, vp, vp, i32], "du_sincos": [vp, vp, vp, i32], "du_round": [vp, vp, vp, vp, vp, vp, i32],
         "du_undistort": [vp, i32, vp, vp, vp]}
_DEVICE = {"du_wave_i32": [i32, vp, vp, i32], "du_wave_u64": [i32, vp, vp, vp, i32], "du_wave_f64": [vp, vp, i32],
           "du_quat": [vp, vp, vp, i32], "du_rotate": [vp, vp, vp, i32], "du_qmul": [vp, vp, vp, i32],
           "du_project": [vp, vp, vp, vp, vp, vp, i32], "du_huber": [vp, vp, vp, i32],
           "du_ldlt6": [vp, vp, vp, vp, i32], "du_ldlt7": [vp, vp, vp, vp, i32],
           "du_block_sum2": [vp, vp, i32], "du_block_sum7": [vp, vp, i32], "du_block_count": [vp, vp, i32],
           "du_decode8": [vp, i32, vp, i32], "du_decode3": [vp, i32, vp, i32], "du_clampn": [vp, vp, vp, i32],
           "du_rigid": [vp, vp, vp, i32], "du_device_count": []}
_POSE = {"du_pose_normalise": [vp, vp, vp, i32], "du_pose_eig": [vp, vp, i32], "du_pose_homography": [vp, vp, vp, i32],
         "du_pose_rotations": [vp, vp, vp, i32], "du_pose_translation": [vp, vp, vp, vp, i32], "du_pose_rot2vec": [vp, vp, i32],
         "du_pose_reproj": [vp, vp, vp, vp, vp, vp, i32], "du_pose_solve": [vp, C.c_float, vp, vp, i32],
         "du_pose_solve_half": [vp, C.c_float, vp, i32, vp, i32]}


def hipcc_command(out, flags=None, source=SOURCE):
    """the hipcc line of a probe (`source`): the library's flags as build() composes them (`flags` replaces them, for a scratch experiment)"""
    hipcc = "hipcc" if subprocess.call(["which", "hipcc"], stdout=subprocess.DEVNULL) == 0 else "/opt/rocm/bin/hipcc"
    if flags is None:
        flags = list(entry.HIPCC_FLAGS) + [f for f in os.environ.get("ORBFE_EXTRA_HIPCC_FLAGS", "").split() if f]
    return [hipcc] + list(flags) + [source, "-o", out]


def _declare(L, table):
    for name, args in table.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_int
    return L


def probe():
    global _probe
    if _probe is None:
        so = os.path.join(tempfile.mkdtemp(prefix="device_units_"), "device_units_probe.so")
        subprocess.check_call(hipcc_command(so))
        _probe = _declare(_declare(_declare(C.CDLL(so), _MATH), _DEVICE), _POSE)
    return _probe


def host():
    global _host
    if _host is None:
        _host = _declare(ref_build.build_shared("device_units_host.cpp", prefix="device_units_host_"), _MATH)
    return _host


def sanitizer_program():
    """the host file as a program of its own under -fsanitize=address,undefined; returns its path"""
    exe = os.path.join(tempfile.mkdtemp(prefix="device_units_san_"), "device_units_san")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-Wall", "-Werror", "-DDEVICE_UNITS_MAIN", os.path.join(ref_build.HERE, "device_units_host.cpp"), "-o", exe])
    return exe


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _in(a, dtype):
    return np.ascontiguousarray(a, dtype)


def _ok(rc, name):
    if rc != 0:
        raise RuntimeError("%s: HIP error %d" % (name, rc))


# ---- include/orbfe_math.h (L = probe() or host())
def atan2(L, y, x):
    y, x = _in(y, np.float32).ravel(), _in(x, np.float32).ravel()
    assert y.shape == x.shape
    out = np.empty(len(y), np.float32)
    _ok(L.du_atan2(_p(y), _p(x), _p(out), len(y)), "du_atan2")
    return out


def sincos(L, a):
    a = _in(a, np.float32).ravel()
    s, c = np.empty(len(a), np.float32), np.empty(len(a), np.float32)
    _ok(L.du_sincos(_p(a), _p(s), _p(c), len(a)), "du_sincos")
    return s, c


def rounders(L, v):
    """orbfe_round_d, orbfe_round_f (on float32(v)), orbfe_floor_d, orbfe_ceil_d of the doubles v"""
    v = _in(v, np.float64).ravel()
    vf = v.astype(np.float32)
    out = [np.empty(len(v), np.int32) for _ in range(4)]
    _ok(L.du_round(_p(v), _p(vf), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), len(v)), "du_round")
    return out


def undistort(L, uv, cam4, k12):
    uv = _in(uv, np.float32).reshape(-1, 2)
    cam4, k12 = _in(cam4, np.float64), _in(k12, np.float64)
    assert cam4.shape == (4,) and k12.shape == (12,)
    out = np.empty_like(uv)
    _ok(L.du_undistort(_p(uv), len(uv), _p(cam4), _p(k12), _p(out)), "du_undistort")
    return out


# ---- csrc/wave_dpp.hpp: rows of 64 values, one wave each
SCAN, ROW16, SUM, MAX, MIN = range(5)
U_MAX, U_MIN, U_MIN2 = range(3)


def wave_i32(op, rows):
    rows = _in(rows, np.int32)
    assert rows.ndim == 2 and rows.shape[1] == 64
    out = np.empty_like(rows)
    _ok(probe().du_wave_i32(op, _p(rows), _p(out), rows.size), "du_wave_i32")
    return out


def wave_u64(op, rows):
    rows = _in(rows, np.uint64)
    assert rows.ndim == 2 and rows.shape[1] == 64
    out, out2 = np.empty_like(rows), np.empty_like(rows)
    _ok(probe().du_wave_u64(op, _p(rows), _p(out), _p(out2), rows.size), "du_wave_u64")
    return (out, out2) if op == U_MIN2 else out


def wave_f64(rows):
    rows = _in(rows, np.float64)
    assert rows.ndim == 2 and rows.shape[1] == 64
    out = np.empty_like(rows)
    _ok(probe().du_wave_f64(_p(rows), _p(out), rows.size), "du_wave_f64")
    return out


# ---- csrc/lm_dense.hpp
def quat(R):
    """quat_from_matrix of n x 3 x 3: (q as x y z w, the matrix rotate() gives for q)"""
    R = _in(R, np.float64).reshape(-1, 3, 3)
    q, rot = np.empty((len(R), 4)), np.empty((len(R), 3, 3))
    _ok(probe().du_quat(_p(R), _p(q), _p(rot), len(R)), "du_quat")
    return q, rot


def rotate(q, v):
    q, v = _in(q, np.float64).reshape(-1, 4), _in(v, np.float64).reshape(-1, 3)
    assert len(q) == len(v)
    r = np.empty_like(v)
    _ok(probe().du_rotate(_p(q), _p(v), _p(r), len(q)), "du_rotate")
    return r


def qmul(a, b):
    a, b = _in(a, np.float64).reshape(-1, 4), _in(b, np.float64).reshape(-1, 4)
    assert len(a) == len(b)
    r = np.empty_like(a)
    _ok(probe().du_qmul(_p(a), _p(b), _p(r), len(a)), "du_qmul")
    return r


def project(Xc, obs, cam4, info):
    Xc, obs, cam4, info = _in(Xc, np.float64).reshape(-1, 3), _in(obs, np.float64).reshape(-1, 2), _in(cam4, np.float64), _in(info, np.float64).ravel()
    assert len(Xc) == len(obs) == len(info) and cam4.shape == (4,)
    err, chi2 = np.empty_like(obs), np.empty(len(Xc))
    _ok(probe().du_project(_p(Xc), _p(obs), _p(cam4), _p(info), _p(err), _p(chi2), len(Xc)), "du_project")
    return err, chi2


def huber(chi2, delta):
    chi2, delta = _in(chi2, np.float64).ravel(), _in(delta, np.float64).ravel()
    assert len(chi2) == len(delta)
    rho = np.empty((len(chi2), 2))
    _ok(probe().du_huber(_p(chi2), _p(delta), _p(rho), len(chi2)), "du_huber")
    return rho


def ldlt(H, b, x0):
    """ldlt_solve<N> of n systems (N = 6 or 7): (ok, x), x starting as x0"""
    H, b = _in(H, np.float64), _in(b, np.float64)
    n, N = b.shape
    assert N in (6, 7) and H.shape == (n, N, N)
    x = np.array(np.broadcast_to(x0, b.shape), np.float64, order="C")
    ok = np.empty(n, np.int32)
    _ok(getattr(probe(), "du_ldlt%d" % N)(_p(H), _p(b), _p(x), _p(ok), n), "du_ldlt%d" % N)
    return ok.astype(bool), x


def block_sum(v):
    """block_sum<N> of nblk x 256 x N (N = 2 or 7): nblk x N"""
    v = _in(v, np.float64)
    nblk, t, N = v.shape
    assert t == 256 and N in (2, 7)
    out = np.empty((nblk, N))
    _ok(getattr(probe(), "du_block_sum%d" % N)(_p(v), _p(out), nblk), "du_block_sum%d" % N)
    return out


def block_count(c):
    c = _in(c, np.int32)
    assert c.ndim == 2 and c.shape[1] == 256
    out = np.empty(len(c), np.int32)
    _ok(probe().du_block_count(_p(c), _p(out), len(c)), "du_block_count")
    return out


# ---- csrc/ransac_sets.hpp
def decode(K, N, words):
    words = _in(words, np.int32).reshape(-1, K)
    assert K in (3, 8) and N >= K
    out = np.empty_like(words)
    _ok(getattr(probe(), "du_decode%d" % K)(_p(words), int(N), _p(out), len(words)), "du_decode%d" % K)
    return out


def clampn(n, cap):
    n, cap = _in(n, np.int32).ravel(), _in(cap, np.int32).ravel()
    assert len(n) == len(cap)
    out = np.empty_like(n)
    _ok(probe().du_clampn(_p(n), _p(cap), _p(out), len(n)), "du_clampn")
    return out


# ---- csrc/sim3_points.hpp
def rigid(T, p):
    T, p = _in(T, np.float32).reshape(-1, 12), _in(p, np.float32).reshape(-1, 3)
    assert len(T) == len(p)
    d = np.empty_like(p)
    _ok(probe().du_rigid(_p(T), _p(p), _p(d), len(T)), "du_rigid")
    return d


# ---- csrc/aruco_pose.hpp: cam17 = fx fy cx cy k[12] has_dist as doubles, one camera per call
def _cam(cam17):
    cam17 = _in(cam17, np.float64)
    assert cam17.shape == (17,)
    return cam17


def pose_normalise(uv, cam17):
    uv, cam17 = _in(uv, np.float32).reshape(-1, 2), _cam(cam17)
    out = np.empty(uv.shape, np.float64)
    _ok(probe().du_pose_normalise(_p(uv), _p(cam17), _p(out), len(uv)), "du_pose_normalise")
    return out


def pose_eig(a6):
    a6 = _in(a6, np.float64).reshape(-1, 6)
    h = np.empty((len(a6), 3))
    _ok(probe().du_pose_eig(_p(a6), _p(h), len(a6)), "du_pose_eig")
    return h


def pose_homography(src, dst):
    src, dst = _in(src, np.float64).reshape(-1, 8), _in(dst, np.float64).reshape(-1, 8)
    assert len(src) == len(dst)
    H = np.empty((len(src), 9))
    _ok(probe().du_pose_homography(_p(src), _p(dst), _p(H), len(src)), "du_pose_homography")
    return H


def pose_rotations(j6):
    j6 = _in(j6, np.float64).reshape(-1, 6)
    R1, R2 = np.empty((len(j6), 9)), np.empty((len(j6), 9))
    _ok(probe().du_pose_rotations(_p(j6), _p(R1), _p(R2), len(j6)), "du_pose_rotations")
    return R1, R2


def pose_translation(obj, img, R):
    obj, img, R = _in(obj, np.float64).reshape(-1, 8), _in(img, np.float64).reshape(-1, 8), _in(R, np.float64).reshape(-1, 9)
    assert len(obj) == len(img) == len(R)
    t = np.empty((len(R), 3))
    _ok(probe().du_pose_translation(_p(obj), _p(img), _p(R), _p(t), len(R)), "du_pose_translation")
    return t


def pose_rot2vec(R):
    R = _in(R, np.float64).reshape(-1, 9)
    r = np.empty((len(R), 3))
    _ok(probe().du_pose_rot2vec(_p(R), _p(r), len(R)), "du_pose_rot2vec")
    return r


def pose_reproj(obj, img, cam17, R, t):
    obj, img = _in(obj, np.float32).reshape(-1, 8), _in(img, np.float32).reshape(-1, 8)
    R, t, cam17 = _in(R, np.float64).reshape(-1, 9), _in(t, np.float64).reshape(-1, 3), _cam(cam17)
    assert len(obj) == len(img) == len(R) == len(t)
    err = np.empty(len(R), np.float32)
    _ok(probe().du_pose_reproj(_p(obj), _p(img), _p(cam17), _p(R), _p(t), _p(err), len(R)), "du_pose_reproj")
    return err


def pose_solve(corners, size, cam17):
    """solve_marker: n x 14 = rvec tvec rvec2 tvec2 err[2]"""
    corners, cam17 = _in(corners, np.float32).reshape(-1, 8), _cam(cam17)
    out = np.empty((len(corners), 14), np.float32)
    _ok(probe().du_pose_solve(_p(corners), np.float32(size), _p(cam17), _p(out), len(corners)), "du_pose_solve")
    return out


def pose_solve_half(corners, size, cam17, which):
    """solve_marker_half: n x 7 = err rvec tvec of solution `which`"""
    corners, cam17 = _in(corners, np.float32).reshape(-1, 8), _cam(cam17)
    out = np.empty((len(corners), 7), np.float32)
    _ok(probe().du_pose_solve_half(_p(corners), np.float32(size), _p(cam17), int(which), _p(out), len(corners)), "du_pose_solve_half")
    return out
