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


MOCK_DIRS = ("tests/mock_orbslam", "tests/mock_orbslam/aruco", "tests/mock_orbslam/dbow2")


def build_shim(shim_ccs, driver_cpp, out_dir):
    """The sources shim_ccs of include/shims/, tests/<driver_cpp> and the mock Frame's static members as one program, against the one
    mock tree tests/mock_orbslam/ and the built library; returns the program's path in out_dir.  The only function that compiles a shim
    program: tests/ is on the include path for the drivers that share tests/shim_driver_io.hpp, and -pthread serves the shims that
    lock Map::mMutexMapUpdate."""
    inc = []
    for d in MOCK_DIRS + ("include", "include/shims", "tests"):
        inc += ["-I", os.path.join(ROOT, d)]
    flags = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-pthread"]
    objs = []
    for src in [os.path.join(ROOT, "include", "shims", cc) for cc in shim_ccs] + [os.path.join(HERE, "mock_orbslam", "Frame_statics.cc")]:
        objs.append(os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0] + ".o"))
        subprocess.check_call(flags + inc + ["-c", src, "-o", objs[-1]])
    exe = os.path.join(out_dir, os.path.splitext(driver_cpp)[0])
    lib_dir = os.path.join(ROOT, "orb_slam2_aruco_amd")
    subprocess.check_call(flags + inc + [os.path.join(HERE, driver_cpp)] + objs + ["-o", exe, "-L", lib_dir, "-lorbfe", "-Wl,-rpath," + lib_dir])
    return exe
