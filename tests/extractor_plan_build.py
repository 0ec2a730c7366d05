"""Builds tests/extractor_plan_driver.cpp (csrc/extractor_plan.hpp behind a C ABI) with g++ and loads it with ctypes (test
infrastructure, in the manner of tests/initializer_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build

_lib = None

LEVEL_FIELDS = ("w", "h", "nCols", "nRows", "wCell", "hCell", "ncells", "quota", "nIni", "out_cap", "resize_tab_ok", "blur_strips")
SCALAR_FIELDS = ("nodecap", "veccap", "keycap_lds", "max_wcell", "max_hcell", "max_ini", "ncells_total", "out_total")


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("extractor_plan_driver.cpp", std="c++17", prefix="extractor_plan_")
        vp, i32 = C.c_void_p, C.c_int
        L.xplan_make.argtypes = [i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32]
        L.xplan_blur_sweep.argtypes = [i32, i32, vp]
        L.xplan_input_layout.argtypes = [i32, i32, C.c_ulonglong, C.c_ulonglong, i32, vp, i32]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def make(rows, cols, scale, inv_scale, quota, gaussian_ed=0):
    """(error code, message, per-level dict of arrays, dict of scalars) of the plan for the constructor tables given."""
    scale = np.ascontiguousarray(scale, np.float32); inv_scale = np.ascontiguousarray(inv_scale, np.float32)
    quota = np.ascontiguousarray(quota, np.int32)
    n = len(scale)
    lv = np.zeros((n, len(LEVEL_FIELDS)), np.int32); sc = np.zeros(len(SCALAR_FIELDS), np.int32)
    msg = C.create_string_buffer(256)
    rc = lib().xplan_make(rows, cols, n, _p(scale), _p(inv_scale), _p(quota), int(gaussian_ed), _p(lv), _p(sc), msg, 256)
    return rc, msg.value.decode(), {f: lv[:, i] for i, f in enumerate(LEVEL_FIELDS)}, {f: int(sc[i]) for i, f in enumerate(SCALAR_FIELDS)}


def blur_sweep(w_first, w_last):
    """(number of refused (width, taps, row rule) combinations, the first of them)."""
    bad = np.zeros(3, np.int32)
    return lib().xplan_blur_sweep(w_first, w_last, _p(bad)), tuple(int(v) for v in bad)


def input_layout(rows, cols, step, frame_stride, nframes):
    """(error code, message) of plan_input_layout for a caller's device frames."""
    msg = C.create_string_buffer(256)
    rc = lib().xplan_input_layout(rows, cols, step, frame_stride, nframes, msg, 256)
    return rc, msg.value.decode()


def level0_read_end(cols, gaussian_ed=0):
    """the byte column behind the last one k_blur7_mfma loads from a row of a `cols`-wide level 0 (-1: tables refused)"""
    return lib().xplan_level0_read_end(cols, gaussian_ed)
