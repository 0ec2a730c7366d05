"""Builds tests/sim3_shim_driver.cpp + include/shims/Sim3Solver_orbfe.cc against the mock headers of tests/mock_sim3/ (which come
before tests/mock_cv/ on the include path; test infrastructure, in the manner of tests/init_shim_build.py)."""
import ref_build


def build(out_dir):
    return ref_build.build_shim("Sim3Solver_orbfe.cc", "sim3_shim_driver.cpp", ("tests/mock_sim3", "tests/mock_cv"), out_dir)
