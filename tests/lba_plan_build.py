"""Builds tests/lba_plan_driver.cpp (csrc/lba_plan.hpp and csrc/ba_camera.hpp behind a C ABI) with g++ and loads it with ctypes, in
the manner of tests/match_plan_build.py; sanitizer_program() builds the same source as a stand-alone program with AddressSanitizer and
UBSan (test infrastructure).  One build per process, in a temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import ref_build

_lib = None

CONSTANTS = ("LBA_MAXV", "LBA_N", "LBA_PT", "LBA_MAX_LEVELS", "LBA_EBLK", "LBA_MBLK", "LBA_SE3_BYTES", "LBA_SOLVE_LDS", "sizeof_ctl", "sizeof_result")
SCRATCH_ARRAYS = ("ctl", "xv", "xl", "e_chi2", "m_chi2", "e_level", "m_level", "pose0", "pose1", "pt0", "pt1", "e_kf", "e_pt", "e_ox", "e_oy",
                  "e_info", "e_use", "e_blk", "mo_marker", "m_use", "m_blk", "Hll", "bl", "Dinv", "p_active", "Hpp", "bp", "vmax", "v_active", "v_kf",
                  "kf_free", "tbl", "S", "bs", "chi_part", "scale_part", "max_part")
IO_ARRAYS = ("fixed", "off", "kf", "xy", "oct", "mloc", "moff", "mkf", "mcor", "T", "X", "M", "erase", "res")
SCHEDULE_FIELDS = ("npb", "nb", "g_setup", "g_pass", "g_points", "g_edges", "vmax", "lds_rows", "tri_bytes", "rounds", "maxit0", "maxit1", "trials",
                   "launches")
# the arrays of a problem as lplan_check_host takes them, with their element types
HOST_ARRAYS = (("Tcw", np.float32), ("kf_fixed", np.uint8), ("x3Dw", np.float32), ("obs_offset", np.int32), ("obs_kf", np.int32),
               ("obs_xy", np.float32), ("obs_octave", np.int32), ("Twm", np.float32), ("marker_local", np.float32), ("mobs_offset", np.int32),
               ("mobs_kf", np.int32), ("mobs_corners", np.float32))
DEVICE_ARGS = ("Tcw", "kf_fixed", "x3Dw", "obs_offset", "obs_kf", "obs_xy", "obs_octave", "obs_feature", "kps", "Twm", "marker_local", "mobs_offset",
               "mobs_kf", "mobs_corners", "erase", "res", "scratch")


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("lba_plan_driver.cpp", std="c++17", prefix="lba_plan_")
        vp, i32, u64 = C.c_void_p, C.c_int, C.c_ulonglong
        L.lplan_constants.argtypes = [vp]
        L.lplan_sizes_ok.argtypes = [vp]
        L.lplan_check_host.argtypes = [vp] * 13 + [i32, i32, vp, i32]
        L.lplan_check_device.argtypes = [vp, vp, i32, u64, vp, i32]
        L.lplan_scratch.argtypes = [vp, vp, vp]
        L.lplan_scratch_bytes.argtypes = [vp]
        L.lplan_scratch_bytes.restype = u64
        L.lplan_host_io.argtypes = [vp, vp, vp]
        L.lplan_schedule.argtypes = [vp, i32, i32, u64, vp]
        L.lplan_camera.argtypes = [C.c_char_p, vp, vp, i32, C.c_float, vp, vp, vp, vp, i32]
        _lib = L
    return _lib


def _sizes(n):
    a = np.array(n, np.int32)
    assert a.shape == (5,)
    return a


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def constants():
    out = np.zeros(len(CONSTANTS), np.int64)
    lib().lplan_constants(_p(out))
    return {f: int(v) for f, v in zip(CONSTANTS, out)}


def sizes_ok(n):
    return bool(lib().lplan_sizes_ok(_p(_sizes(n))))


def check_host(n, arrays, nlevels, use_markers):
    """lba_check_host on the sizes n = (nkf, np, nobs, nma, nmobs) and a dict of arrays (a missing or None entry is NULL); returns
    (code, message)"""
    held = [None if arrays.get(k) is None else np.ascontiguousarray(arrays[k], t) for k, t in HOST_ARRAYS]
    msg = C.create_string_buffer(256)
    s = _sizes(n)
    return lib().lplan_check_host(_p(s), *[_p(a) for a in held], nlevels, use_markers, msg, 256), msg.value.decode()


def check_device(n, addresses, capacity, scratch_bytes):
    """the device call's checks on a dict of addresses (integers; missing = NULL); returns (code, message)"""
    a = np.array([addresses.get(k, 0) for k in DEVICE_ARGS], np.uint64)
    msg = C.create_string_buffer(256)
    s = _sizes(n)
    return lib().lplan_check_device(_p(s), _p(a), capacity, scratch_bytes, msg, 256), msg.value.decode()


def _layout(fn, names, n):
    out, length = np.zeros(len(names) + 3, np.int64), np.zeros(len(names), np.int64)
    s = _sizes(n)
    fn(_p(s), _p(out), _p(length))
    return [(k, int(o), int(b)) for k, o, b in zip(names, out, length)], [int(v) for v in out[len(names):]]


def scratch(n):
    """([(array, offset, the driver's length of it)] in declaration order, dict(zero_end, tbl_bytes, end))"""
    arrays, tail = _layout(lib().lplan_scratch, SCRATCH_ARRAYS, n)
    return arrays, dict(zip(("zero_end", "tbl_bytes", "end"), tail))


def scratch_bytes(n):
    return int(lib().lplan_scratch_bytes(_p(_sizes(n))))


def host_io(n):
    """([(array, offset, length)], dict(split, down, end))"""
    arrays, tail = _layout(lib().lplan_host_io, IO_ARRAYS, n)
    return arrays, dict(zip(("split", "down", "end"), tail))


def schedule(n, use_markers, inspect=False, lds_limit=163840):
    out = np.zeros(len(SCHEDULE_FIELDS), np.int64)
    lib().lplan_schedule(_p(_sizes(n)), int(use_markers), int(inspect), lds_limit, _p(out))
    return {f: int(v) for f, v in zip(SCHEDULE_FIELDS, out)}


def camera(name, K4, inv_sigma2, nlevels, marker_info):
    """ba_camera; returns (code, message, dict(K4, marker_info, nlevels, delta, inv_sigma2 (32)))"""
    K = None if K4 is None else np.ascontiguousarray(K4, np.float32)
    sig = None if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32)
    out, delta, nl, msg = np.zeros(37, np.float32), np.zeros(1, np.float64), np.zeros(1, np.int32), C.create_string_buffer(256)
    rc = lib().lplan_camera(name.encode(), _p(K), _p(sig), nlevels, marker_info, _p(out), _p(delta), _p(nl), msg, 256)
    return rc, msg.value.decode(), dict(K4=out[:4], marker_info=float(out[4]), nlevels=int(nl[0]), delta=float(delta[0]), inv_sigma2=out[5:])


def sanitizer_program():
    """the driver as a program of its own under -fsanitize=address,undefined; returns its path"""
    exe = os.path.join(tempfile.mkdtemp(prefix="lba_plan_san_"), "lba_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-Wall", "-Werror", "-DLBA_PLAN_MAIN", os.path.join(ref_build.HERE, "lba_plan_driver.cpp"), "-o", exe])
    return exe
