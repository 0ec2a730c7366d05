"""Builds the programs of the OptimizeEssentialGraph shim (test infrastructure): include/shims/Optimizer_essential_orbfe.cc with
tests/essential_shim_driver.cpp, and every shim of include/shims/ that shares the one mock tree with tests/all_shims9_driver.cpp, both
against the mock headers of tests/mock_orbslam_eg/ ahead of tests/mock_orbslam/ and the built library."""
import os
import subprocess

import numpy as np

import ref_build
import shim_build

SHIM = "Optimizer_essential_orbfe.cc"
FILES = dict(vk=np.int32, id=np.int32, fixed=np.int32, cpos=np.int32, npos=np.int32, ei=np.int32, ej=np.int32, ek=np.int32, pref=np.int32, Tcw=np.float32,
             x=np.float32, csim=np.float64, nsim=np.float64, threw=np.int32)
RUN_FILES = dict(T=np.float32, P=np.float32, M=np.float32, counts=np.int32)


def build(shim_ccs, driver_cpp, out_dir):
    root, here = ref_build.ROOT, ref_build.HERE
    inc = []
    for d in ("tests/mock_orbslam_eg",) + ref_build.MOCK_DIRS + ("include", "include/shims", "tests"):
        inc += ["-I", os.path.join(root, d)]
    flags = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror"]
    objs = []
    for src in [os.path.join(root, "include", "shims", cc) for cc in shim_ccs] + [os.path.join(here, "mock_orbslam", "Frame_statics.cc")]:
        objs.append(os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0] + ".o"))
        subprocess.check_call(flags + inc + ["-c", src, "-o", objs[-1]])
    exe = os.path.join(out_dir, os.path.splitext(driver_cpp)[0])
    lib_dir = os.path.join(root, "orb_slam2_aruco_amd")
    subprocess.check_call(flags + inc + [os.path.join(here, driver_cpp)] + objs + ["-o", exe, "-L", lib_dir, "-lorbfe", "-Wl,-rpath," + lib_dir])
    return exe


def build_driver(out_dir):
    return build((SHIM,), "essential_shim_driver.cpp", out_dir)


def build_all9(out_dir):
    """the shims of shim_build.PROGRAMS["all"], the LocalMapping shim and this one in one program"""
    return build(tuple(shim_build.PROGRAMS["all"][0]) + ("LocalMapping_orbfe.cc", SHIM), "all_shims9_driver.cpp", out_dir)


def run(exe, mode, out_dir):
    prefix = os.path.join(out_dir, "eg_" + mode)
    subprocess.check_call([exe, mode, prefix])
    kinds = dict(FILES, **(RUN_FILES if mode == "run" else {}))
    return {k: np.fromfile(prefix + "_" + k + ".bin", t) for k, t in kinds.items()}


def problem(d):
    """the dumped flat arrays as a problem binding.eg_arrays takes: what the shim hands the library"""
    return dict(kf_id=d["id"], Tcw=d["Tcw"].reshape(-1, 3, 4), fixed=int(d["fixed"][0]), corrected_pos=d["cpos"], corrected=d["csim"].reshape(-1, 8),
                noncorrected_pos=d["npos"], noncorrected=d["nsim"].reshape(-1, 8), edge_i=d["ei"], edge_j=d["ej"], edge_kind=d["ek"],
                x3Dw=d["x"].reshape(-1, 3), point_ref=d["pref"], iterations=20, fix_scale=1, leaf_vertices=0)
