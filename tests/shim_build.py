"""Builds the shim programs (test infrastructure): the sources of include/shims/ and a driver of tests/, compiled -Wall -Werror against the
one mock ORB-SLAM2 tree tests/mock_orbslam/ and linked against the built library.  "all" links every shim into one program, as an
integration does."""
import ref_build

PROGRAMS = {
    "matcher": (("ORBmatcher_orbfe.cc",), "shim_driver.cpp"),   # with ORBextractor.h and MarkerDetector.h, which the driver includes
    "init": (("Initializer_orbfe.cc",), "init_shim_driver.cpp"),
    "pose": (("Optimizer_pose_orbfe.cc",), "pose_shim_driver.cpp"),
    "sim3": (("Sim3Solver_orbfe.cc",), "sim3_shim_driver.cpp"),
    "sim3_opt": (("Optimizer_sim3_orbfe.cc",), "sim3_opt_shim_driver.cpp"),
    "kfdb": (("KeyFrameDatabase_orbfe.cc",), "kfdb_shim_driver.cpp"),
}
# the shims that have build modules of their own (tests/local_mapping_shim_build.py, essential_shim_build.py, lba_build.py, gba_build.py)
OTHER_SHIMS = ("LocalMapping_orbfe.cc", "Optimizer_essential_orbfe.cc", "Optimizer_localba_orbfe.cc", "Optimizer_globalba_orbfe.cc")
PROGRAMS["all"] = (tuple(cc for name in sorted(PROGRAMS) for cc in PROGRAMS[name][0]) + OTHER_SHIMS, "all_shims_driver.cpp")


def build(name, out_dir):
    """the program's path in out_dir"""
    shim_ccs, driver = PROGRAMS[name]
    return ref_build.build_shim(shim_ccs, driver, out_dir)
