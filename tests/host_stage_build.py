"""Builds tests/host_stage_driver.cpp (the IoLayout of csrc/host_stage.hpp behind a C ABI) with g++ and loads it with ctypes (test
infrastructure, in the manner of tests/detector_plan_build.py)."""
import ctypes as C

import numpy as np

import ref_build


def layout(inputs, outputs):
    """(offsets of the inputs, offsets of the outputs, (upload begin, upload end), (download begin, download end)) of one layout."""
    L = ref_build.build_shared("host_stage_driver.cpp", std="c++17")
    L.iolayout_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.iolayout_run.restype = None
    i = np.ascontiguousarray(inputs, np.int64); o = np.ascontiguousarray(outputs, np.int64)
    off = np.zeros(len(i) + len(o), np.int64); rng = np.zeros(4, np.int64)
    L.iolayout_run(i.ctypes.data, len(i), o.ctypes.data, len(o), off.ctypes.data, rng.ctypes.data)
    return off[:len(i)].tolist(), off[len(i):].tolist(), (int(rng[0]), int(rng[1])), (int(rng[2]), int(rng[3]))
