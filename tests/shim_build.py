"""Builds tests/shim_driver.cpp + include/shims/ORBmatcher_orbfe.cc against the mock headers of tests/mock_cv/ (test infrastructure)."""
import ref_build


def build(out_dir):
    return ref_build.build_shim("ORBmatcher_orbfe.cc", "shim_driver.cpp", ("tests/mock_cv", "tests/mock_cv/orbslam", "tests/mock_cv/aruco"), out_dir)
