"""Builds the LocalMapping shim programs (test infrastructure), through ref_build.build_shim as tests/shim_build.py does for the other
shims: include/shims/LocalMapping_orbfe.cc with its driver."""
import numpy as np

import ref_build

SHIM = "LocalMapping_orbfe.cc"


def build(out_dir):
    """the shim with tests/local_mapping_shim_driver.cpp: the program's path in out_dir"""
    return ref_build.build_shim((SHIM,), "local_mapping_shim_driver.cpp", out_dir)


def write_inputs(prefix, frames, K4, scale, sigma2):
    """the driver's input files for keyframes given as the dicts of tests/new_points_cases.py"""
    def w(name, a, dtype):
        np.ascontiguousarray(a, dtype).tofile(prefix + "_" + name + ".bin")
    w("nf", [len(frames)], np.int32); w("K", K4, np.float32); w("sf", scale, np.float32); w("sg", sigma2, np.float32)
    for f, fr in enumerate(frames):
        w("kps%d" % f, fr["kps"], fr["kps"].dtype); w("desc%d" % f, fr["desc"], np.uint8)
        w("fvn%d" % f, fr["fv"][0], np.uint32); w("fvo%d" % f, fr["fv"][1], np.int32); w("fvf%d" % f, fr["fv"][2], np.uint32)
        w("x%d" % f, fr["x3Dw"], np.float32); w("v%d" % f, fr["valid"], np.uint8); w("T%d" % f, fr["Tcw"], np.float32)


def read_outputs(prefix, neighbours):
    out = []
    for p in range(1, neighbours + 1):
        idx = np.fromfile(prefix + "_i%d.bin" % p, np.int32).reshape(-1, 2)
        out.append((idx[:, 0], idx[:, 1], np.fromfile(prefix + "_x%d.bin" % p, np.float32).reshape(-1, 3)))
    return out
