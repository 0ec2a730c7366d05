"""Builds tests/kfdb_shim_driver.cpp + include/shims/KeyFrameDatabase_orbfe.cc against the mock headers of tests/mock_kfdb/ and its stand-in for DBoW2's BowVector.h, tests/mock_kfdb/dbow2/ (test
infrastructure, in the manner of tests/sim3_opt_shim_build.py)."""
import ref_build


def build(out_dir):
    return ref_build.build_shim("KeyFrameDatabase_orbfe.cc", "kfdb_shim_driver.cpp", ("tests/mock_kfdb", "tests/mock_kfdb/dbow2"), out_dir)
