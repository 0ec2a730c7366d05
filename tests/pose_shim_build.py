"""Builds tests/pose_shim_driver.cpp + include/shims/Optimizer_pose_orbfe.cc against the mock headers of tests/mock_pose/ (which
come before tests/mock_cv/ on the include path; test infrastructure, in the manner of tests/init_shim_build.py)."""
import ref_build


def build(out_dir):
    return ref_build.build_shim("Optimizer_pose_orbfe.cc", "pose_shim_driver.cpp", ("tests/mock_pose", "tests/mock_cv"), out_dir)
