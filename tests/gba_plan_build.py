"""Builds tests/gba_plan_driver.cpp (csrc/gba_plan.hpp behind a C ABI) with g++ and loads it with ctypes, in the manner of
tests/essential_plan_build.py; sanitizer_program() builds the same source as a stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer (test infrastructure)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import ref_build

CONSTANTS = ("GBA_MAXV", "GBA_MAX_OBS", "GBA_LEAF_DEFAULT", "GBA_FRONT_BUDGET", "GBA_SE3_BYTES", "sizeof_ctl", "sizeof_node", "sizeof_src", "sizeof_result",
             "GBA_MAX_ITERATIONS", "GBA_TRIALS")
SCRATCH = ("ctl", "xv", "xt", "xl", "pose0", "pose1", "pt0", "pt1", "e_pt", "e_ox", "e_oy", "e_info", "e_use", "e_blk", "m_use", "m_blk", "Hll", "bl", "Dinv",
           "Hpp", "bp", "vmax", "S", "bs", "chi_part", "scale_part", "max_part", "tables", "fronts")
SCHEDULE = ("npb", "nb", "g_setup", "g_pairs", "nlevels", "back_levels", "lds_rows", "tri_bytes", "iterations", "trials", "launches_trial",
            "launches_iteration", "launches", "host_scratch_bytes")
_lib = None
_p = lambda a: a.ctypes.data_as(C.c_void_p)


def lib():
    global _lib
    if _lib is None:
        _lib = ref_build.build_shared("gba_plan_driver.cpp", std="c++17", prefix="gba_plan_")
    return _lib


def constants():
    out = np.zeros(len(CONSTANTS), np.int64)
    lib().gplan_constants(_p(out))
    return dict(zip(CONSTANTS, out.tolist()))


def _graph(pb):
    """sizes and the graph arrays of a problem dict (tests/gba_cases.py), each with at least one entry so that it has an address"""
    g = lambda k, t: np.ascontiguousarray(np.concatenate([np.asarray(pb.get(k, np.zeros(0)), t).reshape(-1), np.zeros(1, t)]))
    fixed, off, okf, moff, mkf = g("kf_fixed", np.uint8), g("obs_offset", np.int32), g("obs_kf", np.int32), g("mobs_offset", np.int32), g("mobs_kf", np.int32)
    n = np.array([len(fixed) - 1, max(len(off) - 2, 0), len(okf) - 1, max(len(moff) - 2, 0), len(mkf) - 1], np.int32)
    return n, [fixed, off, okf, moff, mkf]


def check_sizes(n, iterations=10, leaf=0):
    msg = C.create_string_buffer(256)
    return lib().gplan_check_sizes(_p(np.asarray(n, np.int32)), int(iterations), int(leaf), msg, 256), msg.value.decode()


def check_graph(pb):
    n, arrs = _graph(pb)
    msg = C.create_string_buffer(256)
    return lib().gplan_check_graph(_p(n), *([_p(a) for a in arrs] + [msg, 256])), msg.value.decode()


def make(pb, leaf=None, use_markers=None):
    """the plan of a problem's graph: dict(rc, msg) when refused, else the counts, per vertex v_kf / v_active / node_of / order_of /
    diag_pair, the edge lists of every vertex, the pairs with their items, per node parent / level / own / boundary (lists of
    vertices) / children / nsrc, level_nodes, src (id, r, c, flags), cmap"""
    n, arrs = _graph(pb)
    leaf = int(pb.get("leaf_vertices", 0)) if leaf is None else int(leaf)
    um = int(pb.get("use_markers", 1 if n[3] else 0)) if use_markers is None else int(use_markers)
    V, nobs, nmobs = int(n[0] + n[3]), int(n[2]), int(n[4])
    kmax = int(np.diff(arrs[1][:n[1] + 1]).max()) if n[1] else 0
    cap = np.array([nobs + 1, 8 * nmobs + 1, V + nobs * (kmax + 1) // 2 + nmobs + 1, nobs * (kmax + 1) // 2 + 1, 4 * nmobs + 1, 36 * V * V + 64, 0, 36 * V * V + 64], np.int64)
    cap[6] = cap[2]
    counts = np.zeros(13, np.int64); vtx = np.zeros(7 * V + 8, np.int32); nodes = np.zeros((2 * V + 3, 8), np.int32)
    eit = np.zeros(cap[0], np.int32); mit = np.zeros(cap[1], np.int32); pairs = np.zeros((cap[2] + 1, 4), np.int32); pit = np.zeros((cap[3], 2), np.int32)
    pmit = np.zeros(cap[4], np.int32); nvtx = np.zeros(cap[5], np.int32); src = np.zeros((cap[6], 4), np.int32); cmap = np.zeros(cap[7], np.int32)
    level_nodes = np.zeros(2 * V + 3, np.int32)
    msg = C.create_string_buffer(256)
    rc = lib().gplan_make(_p(n), *([_p(a) for a in arrs] + [um, leaf, _p(counts), _p(vtx), _p(nodes), _p(cap), _p(eit), _p(mit), _p(pairs), _p(pit), _p(pmit),
                                                            _p(nvtx), _p(src), _p(cmap), _p(level_nodes), msg, 256]))
    if rc:
        return dict(rc=rc, msg=msg.value.decode())
    nv, nfree, npairs, nitems, nmitems, nn, nlevels, _, nsrc, ncmap, max_rows, front_doubles, left_out = counts.tolist()
    eoff, moff = vtx[5 * V:5 * V + nv + 1], vtx[6 * V + 1:6 * V + 1 + nv + 1]
    own = [nvtx[r[4]:r[4] + r[2]].tolist() for r in nodes[:nn]]
    bnd = [nvtx[r[4] + r[2]:r[4] + r[2] + r[3]].tolist() for r in nodes[:nn]]
    return dict(rc=0, nv=nv, nfree_kf=nfree, npairs=npairs, nitems=nitems, nmitems=nmitems, nnodes=nn, nlevels=nlevels, max_rows=max_rows,
                front_doubles=front_doubles, n_left_out=left_out, v_kf=vtx[:nv].copy(), v_active=vtx[V:V + nv].copy(), node_of=vtx[2 * V:2 * V + nv].copy(),
                order_of=vtx[3 * V:3 * V + nv].copy(), diag_pair=vtx[4 * V:4 * V + nv].copy(),
                vtx_edges=[eit[eoff[v]:eoff[v + 1]].tolist() for v in range(nv)], vtx_medges=[mit[moff[v]:moff[v + 1]].tolist() for v in range(nv)],
                pair_u=pairs[:npairs, 0].copy(), pair_v=pairs[:npairs, 1].copy(),
                pair_items=[pit[pairs[q, 2]:pairs[q + 1, 2]].tolist() for q in range(npairs)],
                pair_mitems=[pmit[pairs[q, 3]:pairs[q + 1, 3]].tolist() for q in range(npairs)],
                parent=nodes[:nn, 0].copy(), level=nodes[:nn, 1].copy(), nown=nodes[:nn, 2].copy(), nb=nodes[:nn, 3].copy(), own=own, boundary=bnd,
                children=nodes[:nn, 5:7].copy(), node_nsrc=nodes[:nn, 7].copy(), level_nodes=level_nodes[:nn].copy(), src=src[:nsrc].copy(),
                cmap=cmap[:ncmap].copy())


def scratch(n, leaf=0):
    off = np.zeros(len(SCRATCH), np.uint64); ext = np.zeros(2, np.uint64); sizes = np.zeros(4, np.uint64)
    lib().gplan_scratch(_p(np.asarray(n, np.int32)), int(leaf), _p(off), _p(ext), _p(sizes))
    return dict(zip(SCRATCH, off.tolist())), dict(zip(("zero_end", "end"), ext.tolist())), dict(zip(("bytes", "S", "tables", "fronts"), sizes.tolist()))


def schedule(pb, iterations=10, inspect=False, lds_limit=160 * 1024, leaf=None):
    n, arrs = _graph(pb)
    leaf = int(pb.get("leaf_vertices", 0)) if leaf is None else int(leaf)
    out = np.zeros(len(SCHEDULE), np.int64)
    L = lib()
    L.gplan_schedule.argtypes = [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_longlong, C.c_void_p]
    rc = L.gplan_schedule(_p(n), *([_p(a) for a in arrs] + [int(pb.get("use_markers", 1 if n[3] else 0)), leaf, int(iterations), int(inspect), lds_limit, _p(out)]))
    assert rc == 0, rc
    return dict(zip(SCHEDULE, out.tolist()))


def sanitizer_program():
    """the driver as a program of its own under -fsanitize=address,undefined; returns its path"""
    exe = os.path.join(tempfile.mkdtemp(prefix="gba_plan_san_"), "gba_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-Wall", "-Werror", "-DGBA_PLAN_MAIN", os.path.join(ref_build.HERE, "gba_plan_driver.cpp"), "-o", exe])
    return exe
