"""Builds and runs the program of the OptimizeEssentialGraph shim (test infrastructure): include/shims/Optimizer_essential_orbfe.cc with
tests/essential_shim_driver.cpp, through ref_build.build_shim as tests/shim_build.py does for the other shims."""
import os
import subprocess

import numpy as np

import ref_build

SHIM = "Optimizer_essential_orbfe.cc"
FILES = dict(vk=np.int32, id=np.int32, fixed=np.int32, cpos=np.int32, npos=np.int32, ei=np.int32, ej=np.int32, ek=np.int32, pref=np.int32, Tcw=np.float32,
             x=np.float32, csim=np.float64, nsim=np.float64, threw=np.int32)
RUN_FILES = dict(T=np.float32, P=np.float32, M=np.float32, counts=np.int32)


def build_driver(out_dir):
    return ref_build.build_shim((SHIM,), "essential_shim_driver.cpp", out_dir)


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
