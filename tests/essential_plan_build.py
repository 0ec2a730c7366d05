"""Builds tests/essential_plan_driver.cpp (csrc/essential_plan.hpp behind a C ABI) with g++ and loads it with ctypes, in the manner of
tests/lba_plan_build.py (test infrastructure)."""
import ctypes as C

import numpy as np

import ref_build

CONSTANTS = ("EG_MAXKF", "EG_MAXE", "EG_LEAF_DEFAULT", "EG_FRONT_BUDGET", "EG_SIM3_BYTES", "sizeof_ctl", "sizeof_node", "sizeof_src", "sizeof_result")
SCRATCH = ("ctl", "xv", "xt", "kf_nc", "kf_c", "S0", "est0", "est1", "meas", "e_err", "e_chi", "Ji", "Jj", "Hd", "bv", "Hp", "tables", "fronts")
_lib = None
_p = lambda a: a.ctypes.data_as(C.c_void_p)
_q = lambda a: None if a is None else _p(a)


def lib():
    global _lib
    if _lib is None:
        _lib = ref_build.build_shared("essential_plan_driver.cpp", std="c++17", prefix="essential_plan_")
    return _lib


def constants():
    out = np.zeros(len(CONSTANTS), np.int64)
    lib().eplan_constants(_p(out))
    return dict(zip(CONSTANTS, out.tolist()))


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def check_sizes(n, fixed, iterations=20, leaf=0):
    msg = C.create_string_buffer(256)
    return lib().eplan_check_sizes(_p(np.asarray(n, np.int32)), int(fixed), int(iterations), int(leaf), msg, 256), msg.value.decode()


def check_edges(n, ei, ej, ek, kf_id=None):
    msg = C.create_string_buffer(256)
    ei, ej, ek, kf_id = _i32(ei), _i32(ej), _i32(ek), _i32(kf_id)
    return lib().eplan_check_edges(_p(np.asarray(n, np.int32)), _q(ei), _q(ej), _q(ek), _q(kf_id), msg, 256), msg.value.decode()


def check_values(n, Tcw, cpos, csim, npos, nsim, X, pref):
    msg = C.create_string_buffer(256)
    f = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    arrs = [f(Tcw, np.float32), f(cpos, np.int32), f(csim, np.float64), f(npos, np.int32), f(nsim, np.float64), f(X, np.float32), f(pref, np.int32)]
    return lib().eplan_check_values(_p(np.asarray(n, np.int32)), *([_q(a) for a in arrs] + [msg, 256])), msg.value.decode()


def make(nkf, fixed, ei, ej, leaf=0):
    """the plan of a graph: dict(rc, msg) when refused, else counts, node_of, order_of, per node parent / level / own / boundary (lists of
    vertices) / children / nsrc / front, level_nodes, src (id, r, c, flags), cmap"""
    ei, ej = _i32(ei), _i32(ej)
    cap = 64 * nkf * nkf + 64
    counts = np.zeros(8, np.int64); node_of = np.zeros(nkf, np.int32); order_of = np.zeros(nkf, np.int32)
    nodes = np.zeros((2 * nkf + 2, 8), np.int32); vtx = np.zeros(cap, np.int32); front = np.zeros(2 * nkf + 2, np.int64)
    level_nodes = np.zeros(2 * nkf + 2, np.int32); src = np.zeros((nkf + len(ei) + 1, 4), np.int32); cmap = np.zeros(cap, np.int32)
    msg = C.create_string_buffer(256)
    rc = lib().eplan_make(nkf, len(ei), fixed, _p(ei), _p(ej), leaf, _p(counts), _p(node_of), _p(order_of), _p(nodes), _p(vtx), cap, _p(front), _p(level_nodes),
                          _p(src), _p(cmap), msg, 256)
    if rc:
        return dict(rc=rc, msg=msg.value.decode())
    nn = int(counts[0])
    own = [vtx[r[4]:r[4] + r[2]].tolist() for r in nodes[:nn]]
    bnd = [vtx[r[4] + r[2]:r[4] + r[2] + r[3]].tolist() for r in nodes[:nn]]
    return dict(rc=0, nnodes=nn, nlevels=int(counts[1]), npairs=int(counts[2]), nsrc=int(counts[4]), ncmap=int(counts[5]), max_rows=int(counts[6]),
                front_doubles=int(counts[7]), node_of=node_of, order_of=order_of, parent=nodes[:nn, 0].copy(), level=nodes[:nn, 1].copy(), own=own, boundary=bnd,
                children=nodes[:nn, 5:7].copy(), node_nsrc=nodes[:nn, 7].copy(), front=front[:nn].copy(), level_nodes=level_nodes[:nn].copy(),
                src=src[:int(counts[4])].copy(), cmap=cmap[:int(counts[5])].copy())


def scratch(n, leaf=0):
    off = np.zeros(len(SCRATCH), np.uint64); ext = np.zeros(4, np.uint64); sizes = np.zeros(3, np.uint64)
    lib().eplan_scratch(_p(np.asarray(n, np.int32)), leaf, _p(off), _p(ext), _p(sizes))
    return dict(zip(SCRATCH, off.tolist())), dict(zip(("zero_end", "ff_begin", "ff_end", "end"), ext.tolist())), dict(zip(("bytes", "tables", "fronts"), sizes.tolist()))


def schedule(nkf, fixed, ei, ej, leaf=0, iterations=20, inspect=False, lds_limit=160 * 1024):
    ei, ej = _i32(ei), _i32(ej)
    out = np.zeros(8, np.int64)
    L = lib()
    L.eplan_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    rc = L.eplan_schedule(nkf, len(ei), fixed, _p(ei), _p(ej), leaf, iterations, int(inspect), lds_limit, _p(out))
    assert rc == 0
    return dict(zip(("nlevels", "back_levels", "lds_rows", "tri_bytes", "iterations", "trials", "launches_trial", "launches"), out.tolist()))
