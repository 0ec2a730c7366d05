"""The two g++ builds the test helpers share (test infrastructure): a C++ source of tests/ as a shared library for ctypes
(the CPU restatements *_ref.cpp and the plan drivers *_driver.cpp), and a shim of include/shims/ with its driver as a program."""
import ctypes as C
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_libs = {}


def build_shared(source, std="c++14", prefix=None):
    """tests/<source> compiled into a temporary directory and loaded; one build per process."""
    if source not in _libs:
        stem = os.path.splitext(source)[0]
        so = os.path.join(tempfile.mkdtemp(prefix=prefix or stem + "_"), stem + ".so")
        subprocess.check_call(["g++", "-std=" + std, "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(HERE, source), "-o", so])
        _libs[source] = C.CDLL(so)
    return _libs[source]


def build_shim(shim_cc, driver_cpp, mock_dirs, out_dir):
    """include/shims/<shim_cc> and tests/<driver_cpp>, against the mock headers of mock_dirs (in include-path order) and the built
    library; returns the program's path in out_dir."""
    inc = []
    for d in tuple(mock_dirs) + ("include", "include/shims"):
        inc += ["-I", os.path.join(ROOT, d)]
    obj = os.path.join(out_dir, os.path.splitext(shim_cc)[0] + ".o")
    exe = os.path.join(out_dir, os.path.splitext(driver_cpp)[0])
    flags = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-Wno-unused-function"]
    subprocess.check_call(flags + inc + ["-c", os.path.join(ROOT, "include", "shims", shim_cc), "-o", obj])
    lib_dir = os.path.join(ROOT, "orb_slam2_aruco_amd")
    subprocess.check_call(flags + inc + [os.path.join(HERE, driver_cpp), obj, "-o", exe, "-L", lib_dir, "-lorbfe", "-Wl,-rpath," + lib_dir])
    return exe
