"""Builds tests/init_shim_driver.cpp + include/shims/Initializer_orbfe.cc against the mock headers of tests/mock_init/ (which come
before tests/mock_cv/ on the include path; test infrastructure, in the manner of tests/shim_build.py)."""
import ref_build


def build(out_dir):
    return ref_build.build_shim("Initializer_orbfe.cc", "init_shim_driver.cpp", ("tests/mock_init", "tests/mock_cv"), out_dir)
