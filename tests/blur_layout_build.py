"""Builds tests/blur_layout_driver.cpp (the blurred pyramid's tiled layout of csrc/extractor_plan.hpp behind a C ABI) with g++ and
loads it with ctypes, in the manner of tests/extractor_plan_build.py; sanitizer_program() builds the same source as a stand-alone
program with AddressSanitizer and UBSan (test infrastructure)."""
import ctypes as C
import os
import subprocess
import tempfile

import ref_build

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("blur_layout_driver.cpp", std="c++17", prefix="blur_layout_")
        L.blur_layout_check.argtypes = [C.c_int] * 4
        L.blur_layout_roundtrip.argtypes = [C.c_int] * 4
        L.blur_layout_roundtrip.restype = C.c_longlong
        _lib = L
    return _lib


def check(rows, cols, nfeatures, nlevels):
    """0, or the number of the first layout check that fails (see check_layout in the driver)"""
    return lib().blur_layout_check(rows, cols, nfeatures, nlevels)


def roundtrip(rows, cols, nfeatures, nlevels):
    """pixels that differ after filling a frame's blurred block through the address function and de-tiling it (-1: no plan)"""
    return lib().blur_layout_roundtrip(rows, cols, nfeatures, nlevels)


def tile_shape():
    """(bytes of a row, rows) of a 128-byte tile"""
    tw, th = C.c_int(), C.c_int()
    lib().blur_layout_tile(C.byref(tw), C.byref(th))
    return tw.value, th.value


def sanitizer_program():
    """the driver as a program of its own under -fsanitize=address,undefined; returns its path"""
    exe = os.path.join(tempfile.mkdtemp(prefix="blur_layout_san_"), "blur_layout_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-Wall", "-Werror", "-DBLUR_LAYOUT_MAIN", os.path.join(ref_build.HERE, "blur_layout_driver.cpp"), "-o", exe])
    return exe
