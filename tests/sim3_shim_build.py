"""Builds tests/sim3_shim_driver.cpp + include/shims/Sim3Solver_orbfe.cc against the mock headers of tests/mock_sim3/ (which come
before tests/mock_cv/ on the include path; test infrastructure, in the manner of tests/init_shim_build.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(out_dir):
    inc = []
    for d in ("tests/mock_sim3", "tests/mock_cv", "include", "include/shims"):
        inc += ["-I", os.path.join(ROOT, d)]
    obj = os.path.join(out_dir, "shim_sim3solver.o")
    exe = os.path.join(out_dir, "sim3_shim_driver")
    flags = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-Wno-unused-function"]
    subprocess.check_call(flags + inc + ["-c", os.path.join(ROOT, "include", "shims", "Sim3Solver_orbfe.cc"), "-o", obj])
    lib_dir = os.path.join(ROOT, "orb_slam2_aruco_amd")
    subprocess.check_call(flags + inc + [os.path.join(HERE, "sim3_shim_driver.cpp"), obj, "-o", exe, "-L", lib_dir, "-lorbfe",
                                          "-Wl,-rpath," + lib_dir])
    return exe
