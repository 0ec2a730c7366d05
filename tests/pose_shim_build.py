"""Builds tests/pose_shim_driver.cpp + include/shims/Optimizer_pose_orbfe.cc against the mock headers of tests/mock_pose/ (which
come before tests/mock_cv/ on the include path; test infrastructure, in the manner of tests/init_shim_build.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build(out_dir):
    inc = []
    for d in ("tests/mock_pose", "tests/mock_cv", "include", "include/shims"):
        inc += ["-I", os.path.join(ROOT, d)]
    obj = os.path.join(out_dir, "shim_pose.o")
    exe = os.path.join(out_dir, "pose_shim_driver")
    flags = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-Wno-unused-function"]
    subprocess.check_call(flags + inc + ["-c", os.path.join(ROOT, "include", "shims", "Optimizer_pose_orbfe.cc"), "-o", obj])
    lib_dir = os.path.join(ROOT, "orb_slam2_aruco_amd")
    subprocess.check_call(flags + inc + [os.path.join(HERE, "pose_shim_driver.cpp"), obj, "-o", exe, "-L", lib_dir, "-lorbfe",
                                          "-Wl,-rpath," + lib_dir])
    return exe
