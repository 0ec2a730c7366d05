"""Builds the second unit probe, of the optimizers' and solvers' device helpers (test infrastructure, next to device_units_build.py).

probe()  tests/solver_units_probe.hip, compiled once per process into a temporary directory with hipcc and exactly the flags build()
         gives the library's sources (device_units_build.hipcc_command), loaded with ctypes.  The probe includes
         csrc/{se3_quat,sim3_group,svd_jacobi,front_solve,ba_edges}.hpp unchanged; it is not part of liborbfe.so.
host()   the CPU restatements of the same helpers (glibc's libm, g++ -ffp-contract=off) through ref_build.build_shared:
         tests/solver_units_host.cpp (the SE3Quat of g2o_ref.hpp; the passes' shared steps, sequentially), essential_ref.cpp
         (g2o::Sim3), initializer_ref.cpp (jacobi_svd),
         lba_ref.cpp (the marker edge).

The wrappers take and return numpy arrays.  Where a helper has both sides the first argument `L` is probe() or host(); the Sim3 and SVD
wrappers take `device` instead, since their restatements are single calls.  A HIP error code other than 0 raises."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np

import device_units_build as D
import ref_build
import solver_units_cases

_probe = None
_host = None
SOURCE = os.path.join(ref_build.HERE, "solver_units_probe.hip")
GUARD = 64           # doubles before and behind M and r in front_llt
vp, i32 = C.c_void_p, C.c_int
_SE3 = {"su_se3_exp": [vp, vp, i32], "su_se3_mul": [vp, vp, vp, i32], "su_se3_map": [vp, vp, vp, i32], "su_normalize": [vp, vp, i32],
        "su_se3_from_float": [vp, vp, i32], "su_to_float": [vp, vp, i32]}
_DEVICE = {"su_device_count": [], "su_lm_threads": [], "su_sim3_exp": [vp, vp, i32], "su_sim3_log": [vp, vp, i32], "su_sim3_mul": [vp, vp, vp, i32],
           "su_sim3_map": [vp, vp, vp, i32], "su_sim3_inverse": [vp, vp, i32], "su_lu3": [vp, vp, vp, i32],
           "su_svd_3x3": [vp, vp, vp, vp, i32], "su_svd_4x4": [vp, vp, vp, vp, i32], "su_svd_16x9": [vp, vp, vp, vp, i32],
           "su_svd_9x8": [vp, vp, vp, vp, i32], "su_front_llt": [i32, vp, i32, i32, vp, i32, i32, vp, vp],
           "su_front_back6": [i32, i32, i32, i32, vp, vp, vp, vp], "su_front_back7": [i32, i32, i32, i32, vp, vp, vp, vp],
           "su_mono": [vp, vp, vp, vp, vp, i32], "su_marker": [vp, vp, vp, vp, vp, vp, i32], "su_diag": [vp, vp, i32],
           "su_rot_of": [vp, vp, i32], "su_wave": [i32, vp, vp, i32]}
# the shared steps of the passes: on both sides (L = probe() or host())
_PASSES = {"su_lm_threads": [], "su_dinv3": [vp, vp, i32], "su_pair_items": [vp, vp, vp, i32, i32, vp, vp, i32],
           "su_merge": [i32, vp, i32, vp, i32, vp, i32, i32], "su_run_sum": [vp, i32, vp]}
SVD_SHAPES = solver_units_cases.SVD_SHAPES      # (M, N, N1, WANT_U) of the four product instantiations of svd_jacobi


def compile_probe(so):
    subprocess.check_call(D.hipcc_command(so, source=SOURCE))
    return so


def probe():
    global _probe
    if _probe is None:
        so = compile_probe(os.path.join(tempfile.mkdtemp(prefix="solver_units_"), "solver_units_probe.so"))
        _probe = D._declare(D._declare(D._declare(C.CDLL(so), _SE3), _DEVICE), _PASSES)
    return _probe


def host():
    """the restatements: .se3 (the array calls of the SE3Quat group), .eg, .init, .lba"""
    global _host
    if _host is None:
        eg = ref_build.build_shared("essential_ref.cpp")
        for name, args in {"ref_eg_exp": [vp, vp], "ref_eg_log": [vp, vp], "ref_eg_mul": [vp, vp, vp], "ref_eg_inverse": [vp, vp],
                           "ref_eg_map": [vp, vp, vp], "ref_eg_lu3": [vp, vp, vp]}.items():
            getattr(eg, name).argtypes, getattr(eg, name).restype = args, None
        init = ref_build.build_shared("initializer_ref.cpp")
        init.ref_jacobi_svd.argtypes, init.ref_jacobi_svd.restype = [vp, i32, i32, i32, vp, vp], None
        lba = ref_build.build_shared("lba_ref.cpp")
        lba.ref_ba_marker_edge.argtypes, lba.ref_ba_marker_edge.restype = [vp] * 8, None
        se3 = D._declare(D._declare(ref_build.build_shared("solver_units_host.cpp", prefix="solver_units_host_"), _SE3), _PASSES)
        _host = types.SimpleNamespace(se3=se3, eg=eg, init=init, lba=lba)
    return _host


_p, _in, _ok = D._p, D._in, D._ok


def _se3lib(L):
    return L.se3 if isinstance(L, types.SimpleNamespace) else L


def _call(fn, name, widths, wout, *arrays, dtype_out=np.float64):
    ins = [_in(a, np.float64).reshape(-1, w) for a, w in zip(arrays, widths)]
    n = len(ins[0])
    assert all(len(a) == n for a in ins)
    out = np.empty((n, wout), dtype_out)
    _ok(fn(*([_p(a) for a in ins] + [_p(out), n])), name)
    return out


# ---- csrc/se3_quat.hpp (L = probe() or host()); an SE3 is q (x y z w), t
def se3_exp(L, u):
    return _call(_se3lib(L).su_se3_exp, "su_se3_exp", (6,), 7, u)


def se3_mul(L, a, b):
    return _call(_se3lib(L).su_se3_mul, "su_se3_mul", (7, 7), 7, a, b)


def se3_map(L, a, p):
    return _call(_se3lib(L).su_se3_map, "su_se3_map", (7, 3), 3, a, p)


def normalize(L, q):
    return _call(_se3lib(L).su_normalize, "su_normalize", (4,), 4, q)


def se3_from_float(L, Rt):
    Rt = _in(Rt, np.float32).reshape(-1, 12)
    out = np.empty((len(Rt), 7))
    _ok(_se3lib(L).su_se3_from_float(_p(Rt), _p(out), len(Rt)), "su_se3_from_float")
    return out


def to_float(L, a):
    a = _in(a, np.float64).reshape(-1, 7)
    out = np.empty((len(a), 12), np.float32)
    _ok(_se3lib(L).su_to_float(_p(a), _p(out), len(a)), "su_to_float")
    return out


# ---- csrc/sim3_group.hpp; a Sim3 is q (x y z w), t, s
def _each(fn, wout, *arrays):
    out = np.empty((len(arrays[0]), wout))
    for i in range(len(out)):
        fn(*([_p(a[i]) for a in arrays] + [_p(out[i])]))
    return out


def _sim(name, ref, widths, wout, device, *arrays):
    if device:
        return _call(getattr(probe(), name), name, widths, wout, *arrays)
    return _each(getattr(host().eg, ref), wout, *[_in(a, np.float64).reshape(-1, w) for a, w in zip(arrays, widths)])


def sim3_exp(device, u):
    return _sim("su_sim3_exp", "ref_eg_exp", (7,), 8, device, u)


def sim3_log(device, s):
    return _sim("su_sim3_log", "ref_eg_log", (8,), 7, device, s)


def sim3_mul(device, a, b):
    return _sim("su_sim3_mul", "ref_eg_mul", (8, 8), 8, device, a, b)


def sim3_map(device, a, p):
    return _sim("su_sim3_map", "ref_eg_map", (8, 3), 3, device, a, p)


def sim3_inverse(device, a):
    return _sim("su_sim3_inverse", "ref_eg_inverse", (8,), 8, device, a)


def lu3(device, m, b):
    with np.errstate(all="ignore"):
        return _sim("su_lu3", "ref_eg_lu3", (9, 3), 3, device, m, b)


# ---- csrc/svd_jacobi.hpp
def svd(device, shape, At):
    """svd_jacobi<M, N, N1, WANT_U> of At (n x N1 x M float, the transposed inputs with their storage rows): W n x N, Vt n x N x N and At
    behind the call (rows 0..N1-1 are U^T when WANT_U)"""
    M, N, N1, _ = SVD_SHAPES[shape]
    At = _in(At, np.float32)
    n = len(At)
    assert At.shape == (n, N1, M)
    W, Vt, out = np.empty((n, N), np.float32), np.empty((n, N, N), np.float32), np.empty_like(At)
    if device:
        _ok(getattr(probe(), "su_svd_" + shape)(_p(At), _p(W), _p(Vt), _p(out), n), "su_svd_" + shape)
    else:
        out[:] = At
        for i in range(n):
            host().init.ref_jacobi_svd(_p(out[i]), M, N, N1, _p(W[i]), _p(Vt[i]))
    return W, Vt, out


# ---- csrc/front_solve.hpp
def front_llt(packed, M, k, r):
    """front_partial_llt<packed> of nsys systems M (nsys x n x n, rows of n) with right-hand sides r (nsys x n), a workgroup each:
    (M, r, ret nsys x LM_THREADS, fail_s nsys, guards_kept)"""
    M, r = _in(M, np.float64), _in(r, np.float64)
    nsys, n = r.shape
    assert M.shape == (nsys, n, n) and 0 <= k <= n
    rng = np.random.default_rng(99)
    gm, gr = rng.uniform(1, 2, 2 * GUARD), rng.uniform(1, 2, 2 * GUARD)
    m = np.concatenate([gm[:GUARD], M.ravel(), gm[GUARD:]])
    rr = np.concatenate([gr[:GUARD], r.ravel(), gr[GUARD:]])
    ret, fail = np.full((nsys, probe().su_lm_threads()), -1, np.int32), np.full(nsys, -1, np.int32)     # LM_THREADS as the probe was compiled
    _ok(probe().su_front_llt(int(bool(packed)), _p(m), n, int(k), _p(rr), nsys, GUARD, _p(ret), _p(fail)), "su_front_llt")
    kept = (np.array_equal(m[:GUARD], gm[:GUARD]) and np.array_equal(m[-GUARD:], gm[GUARD:]) and np.array_equal(rr[:GUARD], gr[:GUARD])
            and np.array_equal(rr[-GUARD:], gr[GUARD:]))
    return m[GUARD:-GUARD].reshape(nsys, n, n), rr[GUARD:-GUARD].reshape(nsys, n), ret, fail, kept


def front_back(R, nown, nb, vtx, xt, F, r):
    """front_substitute_back<R> of nsys systems of one shape: vtx nsys x (nown + nb), xt nsys x nvert x R (returned), F nsys x n x n, r
    nsys x n"""
    vtx, xt, F, r = _in(vtx, np.int32), np.array(xt, np.float64, order="C"), _in(F, np.float64), _in(r, np.float64)
    nsys, nvert = xt.shape[:2]
    n = R * (nown + nb)
    assert R in (6, 7) and vtx.shape == (nsys, nown + nb) and xt.shape == (nsys, nvert, R) and F.shape == (nsys, n, n) and r.shape == (nsys, n)
    assert vtx.min() >= 0 and vtx.max() < nvert
    _ok(getattr(probe(), "su_front_back%d" % R)(nsys, nown, nb, nvert, _p(vtx), _p(xt), _p(F), _p(r)), "su_front_back%d" % R)
    return xt


# ---- csrc/ba_edges.hpp
def mono(T7, X, obs, cam4):
    """lba_mono_linearize: err n x 2, Jp n x 2 x 6, Jx n x 2 x 3"""
    T7, X, obs, cam4 = _in(T7, np.float64).reshape(-1, 7), _in(X, np.float64).reshape(-1, 3), _in(obs, np.float64).reshape(-1, 2), _in(cam4, np.float64)
    n = len(T7)
    assert len(X) == n == len(obs) and cam4.shape == (4,)
    out = np.empty((n, 20))
    _ok(probe().su_mono(_p(T7), _p(X), _p(obs), _p(cam4), _p(out), n), "su_mono")
    return out[:, :2], out[:, 2:14].reshape(n, 2, 6), out[:, 14:].reshape(n, 2, 3)


def marker(device, Tcw, Twm, p, obs, cam4):
    """lba_marker_error and both lba_marker_jacobian of poses given as 3 x 4 floats: err n x 2, Jc n x 2 x 6, Jm n x 2 x 6"""
    Tcw, Twm = _in(Tcw, np.float32).reshape(-1, 12), _in(Twm, np.float32).reshape(-1, 12)
    p, obs, cam4 = _in(p, np.float64).reshape(-1, 3), _in(obs, np.float64).reshape(-1, 2), _in(cam4, np.float64)
    n = len(Tcw)
    assert len(Twm) == n == len(p) == len(obs) and cam4.shape == (4,)
    out = np.empty((n, 26))
    if device:
        _ok(probe().su_marker(_p(Tcw), _p(Twm), _p(p), _p(obs), _p(cam4), _p(out), n), "su_marker")
    else:
        K4 = cam4.astype(np.float32)
        assert np.array_equal(K4.astype(np.float64), cam4), "the restatement takes the camera as floats"
        for i in range(n):
            host().lba.ref_ba_marker_edge(_p(Tcw[i]), _p(Twm[i]), _p(p[i]), _p(obs[i]), _p(K4), _p(out[i, :2]), _p(out[i, 2:14]), _p(out[i, 14:]))
    return out[:, :2], out[:, 2:14].reshape(n, 2, 6), out[:, 14:].reshape(n, 2, 6)


def diag_block(J, w, r0, r1):
    J = _in(J, np.float64).reshape(-1, 12)
    return _call(probe().su_diag, "su_diag", (15,), 27, np.concatenate([J, np.stack([w, r0, r1], 1)], 1))


def rot_of(q):
    return _call(probe().su_rot_of, "su_rot_of", (4,), 9, q).reshape(-1, 3, 3)


# ---- the steps the passes share (L = probe() or host()): csrc/ba_edges.hpp, front_solve.hpp, lm_dense.hpp
def dinv3(L, H6, lam):
    """damped_inverse3: (Hll + lambda I)^-1 of n packed upper triangles, n x 3 x 3"""
    H6 = _in(H6, np.float64).reshape(-1, 6)
    return _call(_se3lib(L).su_dinv3, "su_dinv3", (7,), 9, np.concatenate([H6, _in(lam, np.float64).reshape(-1, 1)], 1)).reshape(-1, 3, 3)


def pair_items(L, Wi, Wj, Dm, bl, diag, acc, accb):
    """pair_item_add over the items of nsys systems, item after item: Wi, Wj nsys x nitems x 6 x 3, Dm nsys x nitems x 3 x 3, bl nsys x
    nitems x 3; acc nsys x 6 x 6 and accb nsys x 6 are the accumulators' starts; returns them behind the items"""
    Wi, Wj, Dm, bl = _in(Wi, np.float64), _in(Wj, np.float64), _in(Dm, np.float64), _in(bl, np.float64)
    nsys, nitems = Wi.shape[:2]
    assert Wi.shape == Wj.shape == (nsys, nitems, 6, 3) and Dm.shape == (nsys, nitems, 3, 3) and bl.shape == (nsys, nitems, 3)
    w = np.ascontiguousarray(np.concatenate([Wi.reshape(nsys, nitems, 18), Wj.reshape(nsys, nitems, 18)], 2))
    acc, accb = np.array(acc, np.float64, order="C"), np.array(accb, np.float64, order="C")
    assert acc.shape == (nsys, 6, 6) and accb.shape == (nsys, 6)
    _ok(_se3lib(L).su_pair_items(_p(w), _p(Dm), _p(bl), nitems, int(bool(diag)), _p(acc), _p(accb), nsys), "su_pair_items")
    return acc, accb


def merge(L, R, desc, cmap, fronts, node):
    """front_merge_children<R> of node `node`: desc nn x 7 (front offset, nown, nb, child[2], cmap[2]), fronts the doubles of every front
    (returned).  Every front, every child and every map entry is checked to lie inside before the call."""
    desc, cmap, fronts = _in(desc, np.int32), _in(cmap, np.int32), np.array(fronts, np.float64, order="C")
    nn = len(desc)
    assert R in (6, 7) and desc.shape == (nn, 7) and 0 <= node < nn
    for off, nown, nb, c0, c1, m0, m1 in desc:
        n = R * (nown + nb)
        assert 0 <= off and off + n * n + 2 * n <= len(fronts) and nown >= 0 and nb >= 0
        for c, m in ((c0, m0), (c1, m1)):
            assert -1 <= c < nn
            if c >= 0:
                assert 0 <= m and m + desc[c][2] <= len(cmap) and (0 <= cmap[m:m + desc[c][2]]).all() and (cmap[m:m + desc[c][2]] < nown + nb).all()
    _ok(_se3lib(L).su_merge(R, _p(desc), nn, _p(cmap), len(cmap), _p(fronts), len(fronts), node), "su_merge")
    return fronts


def run_sum(L, v):
    """run_sum followed by block_sum over one workgroup"""
    v = _in(v, np.float64).ravel()
    out = np.full(1, np.nan)
    _ok(_se3lib(L).su_run_sum(_p(v), len(v), _p(out)), "su_run_sum")
    return out[0]


SUM, MAX = 0, 1


def wave(op, rows):
    rows = _in(rows, np.float64)
    assert rows.ndim == 2 and rows.shape[1] == 64
    out = np.empty_like(rows)
    _ok(probe().su_wave(op, _p(rows), _p(out), rows.size), "su_wave")
    return out
