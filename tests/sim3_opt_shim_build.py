"""Builds tests/sim3_opt_shim_driver.cpp + include/shims/Optimizer_sim3_orbfe.cc against the mock headers of tests/mock_optsim3/
(which come before tests/mock_cv/ on the include path; test infrastructure, in the manner of tests/sim3_shim_build.py)."""
import ref_build


def build(out_dir):
    return ref_build.build_shim("Optimizer_sim3_orbfe.cc", "sim3_opt_shim_driver.cpp", ("tests/mock_optsim3", "tests/mock_cv"), out_dir)
