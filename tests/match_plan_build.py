"""Builds tests/match_plan_driver.cpp (csrc/match_plan.hpp behind a C ABI) with g++ and loads it with ctypes, in the manner of
tests/pipeline_plan_build.py; sanitizer_program() builds the same source as a stand-alone program with AddressSanitizer and UBSan
(test infrastructure).  One build per process, in a temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import ref_build

_lib = None

CONSTANTS = ("KNN_TILE", "KM_WAVES", "KM_CHUNK", "SFI_MAXL0", "SFI_CURSOR_PAD", "GRID_COLS", "GRID_ROWS", "SBP_CELLS", "MATCH_LDS_LIMIT")
KNN2_FIELDS = ("mfma", "nsplit", "chunk", "scan_x", "scan_y", "scan_z", "scan_block", "merge_x", "merge_y", "merge_z", "part_bytes")
SFI_FIELDS = ("nframes", "pool", "cnt_bytes", "idx_bytes", "dist_bytes", "scratch_bytes", "nl0", "nq", "cursor", "desc", "xy", "sorted", "qxy",
              "ang", "query")
SFI_FLAG_FIELDS = ("need", "err", "pool", "clear")
LDS_FIELDS = ("sorted", "xy", "cell0", "lvl", "taken", "end")
SBP_FIELDS = ("err", "ncap", "lds_bytes") + tuple("lds_" + f for f in LDS_FIELDS) + ("stride", "rank_bytes", "dist_bytes", "cnt_bytes")
FUSE_FIELDS = ("q_bytes", "obest_bytes", "best_level", "second_dist", "second_level", "match", "nq", "nmatches")


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("match_plan_driver.cpp", std="c++17", prefix="match_plan_")
        vp, i32 = C.c_void_p, C.c_int
        L.mplan_constants.argtypes = [vp]
        L.mplan_knn2.argtypes = [i32] * 5 + [vp]
        L.mplan_sfi.argtypes = [i32, i32, vp]
        L.mplan_sfi_pool_after.argtypes = [i32, i32]
        L.mplan_sfi_flags.argtypes = [i32, i32, i32, vp]
        L.mplan_sbp_lds_offsets.argtypes = [i32, vp]
        L.mplan_sbp.argtypes = [i32] * 4 + [vp, vp, i32]
        L.mplan_sbp_stride_after.argtypes = [i32, i32]
        L.mplan_fuse_batch.argtypes = [i32, i32, vp]
        L.mplan_knn2_sweep.argtypes = [vp]
        _lib = L
    return _lib


def _call(fn, fields, dtype, *args):
    out = np.zeros(len(fields), dtype)
    fn(*args, out.ctypes.data_as(C.c_void_p))
    return {f: int(v) for f, v in zip(fields, out)}


def constants():
    return _call(lib().mplan_constants, CONSTANTS, np.int64)


def knn2(max_nq, max_nt, npairs, init=256, path=0):
    """plan_knn2 as a dict; "scan" and "merge" are the grids as tuples, merge None when there is none"""
    p = _call(lib().mplan_knn2, KNN2_FIELDS, np.int64, max_nq, max_nt, npairs, init, path)
    p["scan"] = (p["scan_x"], p["scan_y"], p["scan_z"])
    p["merge"] = (p["merge_x"], p["merge_y"]) if p["merge_x"] else None
    return p


def knn2_sweep():
    """(plans made, plans that break a covering property) over the driver's own sweep"""
    n = C.c_int()
    bad = lib().mplan_knn2_sweep(C.byref(n))
    return n.value, bad


def sfi(npairs, pool_now=0):
    return _call(lib().mplan_sfi, SFI_FIELDS, np.int64, npairs, pool_now)


def sfi_pool_after(now, needed):
    return lib().mplan_sfi_pool_after(now, needed)


def sfi_flags(level0, pool_needed, pool_now):
    return _call(lib().mplan_sfi_flags, SFI_FLAG_FIELDS, np.int32, level0, pool_needed, pool_now)


def sbp_lds_offsets(ncap):
    return _call(lib().mplan_sbp_lds_offsets, LDS_FIELDS, np.int32, ncap)


def sbp(capacity, qcapacity=100, nframes=1, stride_now=0):
    out = np.zeros(len(SBP_FIELDS), np.int64)
    msg = C.create_string_buffer(256)
    lib().mplan_sbp(capacity, qcapacity, nframes, stride_now, out.ctypes.data_as(C.c_void_p), msg, 256)
    l = {f: int(v) for f, v in zip(SBP_FIELDS, out)}
    l["msg"] = msg.value.decode()
    return l


def sbp_stride_after(now, overflow):
    return lib().mplan_sbp_stride_after(now, overflow)


def fuse_batch(nkf, nmp):
    return _call(lib().mplan_fuse_batch, FUSE_FIELDS, np.int64, nkf, nmp)


def sanitizer_program():
    """the driver as a program of its own under -fsanitize=address,undefined; returns its path"""
    exe = os.path.join(tempfile.mkdtemp(prefix="match_plan_san_"), "match_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-Wall", "-Werror", "-DMATCH_PLAN_MAIN", os.path.join(ref_build.HERE, "match_plan_driver.cpp"), "-o", exe])
    return exe
