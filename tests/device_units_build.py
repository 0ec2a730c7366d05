"""Builds the unit probe of the shared device helpers (test infrastructure, in the manner of tests/blur_layout_build.py).

probe()             tests/device_units_probe.hip, compiled once per process into a temporary directory with hipcc and exactly the flags
                    build() gives the library's sources (__graft_entry__.HIPCC_FLAGS + ORBFE_EXTRA_HIPCC_FLAGS), loaded with ctypes.
                    The probe includes include/orbfe_math.h and csrc/{wave_dpp,lm_dense,ransac_sets,sim3_points}.hpp unchanged; it is
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


def hipcc_command(out, flags=None):
    """the hipcc line of the probe: the library's flags as build() composes them (`flags` replaces them, for a scratch experiment)"""
    hipcc = "hipcc" if subprocess.call(["which", "hipcc"], stdout=subprocess.DEVNULL) == 0 else "/opt/rocm/bin/hipcc"
    if flags is None:
        flags = list(entry.HIPCC_FLAGS) + [f for f in os.environ.get("ORBFE_EXTRA_HIPCC_FLAGS", "").split() if f]
    return [hipcc] + list(flags) + [SOURCE, "-o", out]


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
        _probe = _declare(_declare(C.CDLL(so), _MATH), _DEVICE)
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
