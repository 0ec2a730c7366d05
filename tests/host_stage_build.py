"""Builds tests/host_stage_driver.cpp (the IoLayout of csrc/host_stage.hpp behind a C ABI) with g++ and loads it with ctypes (test
infrastructure, in the manner of tests/detector_plan_build.py)."""
import ctypes as C

import numpy as np

import ref_build


def layout3(inputs, inouts, outputs):
    """(offsets of the inputs, of the arrays that travel both ways, of the outputs, (upload begin, upload end), (download begin,
    download end)) of one layout; inouts None: the layout is built without the in-out mark."""
    L = ref_build.build_shared("host_stage_driver.cpp", std="c++17")
    L.iolayout_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.iolayout_run.restype = None
    i, b, o = (np.ascontiguousarray(a if a is not None else [], np.int64) for a in (inputs, inouts, outputs))
    off = np.zeros(len(i) + len(b) + len(o), np.int64); rng = np.zeros(4, np.int64)
    L.iolayout_run(i.ctypes.data, len(i), b.ctypes.data, -1 if inouts is None else len(b), o.ctypes.data, len(o), off.ctypes.data, rng.ctypes.data)
    ni, nb = len(i), len(i) + len(b)
    return off[:ni].tolist(), off[ni:nb].tolist(), off[nb:].tolist(), (int(rng[0]), int(rng[1])), (int(rng[2]), int(rng[3]))


def layout(inputs, outputs):
    """(offsets of the inputs, offsets of the outputs, (upload begin, upload end), (download begin, download end)) of one layout."""
    i_off, _, o_off, up, down = layout3(inputs, None, outputs)
    return i_off, o_off, up, down
