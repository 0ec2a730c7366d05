"""Builds tests/pipeline_plan_driver.cpp (csrc/pipeline_plan.hpp behind a C ABI) with g++ and loads it with ctypes (test
infrastructure, in the manner of tests/extractor_plan_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build

_lib = None

CONFIG_FIELDS = ("engine_sets", "record_sets", "phase_pin", "det_pin", "defer_post", "det_nofork")
SCHEDULE_FIELDS = ("D", "R", "phase_pin", "det_pin", "defer_post", "det_nofork", "describe_late", "gather_stream")


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("pipeline_plan_driver.cpp", std="c++17", prefix="pipeline_plan_")
        vp, i32 = C.c_void_p, C.c_int
        L.pplan_schedule.argtypes = [i32, i32, i32, vp, vp, vp, i32, vp, vp, i32]
        L.pplan_env_defaults.restype = C.c_char_p
        _lib = L
    return _lib


def schedule(rows, cols, use_orb=True, env=None, **config):
    """(plan_schedule's result as a dict, the list of variable names it asked its lookup for).  env: a dict that stands for the
    environment (the process environment is not touched); keyword arguments: fields of the configuration, -1 where not given."""
    env = env or {}
    assert set(config) <= set(CONFIG_FIELDS), config
    cfg = np.array([config.get(f, -1) for f in CONFIG_FIELDS], np.int32)
    names = (C.c_char_p * max(len(env), 1))(*[k.encode() for k in env])
    values = (C.c_char_p * max(len(env), 1))(*[v.encode() for v in env.values()])
    out = np.zeros(len(SCHEDULE_FIELDS), np.int32)
    asked = C.create_string_buffer(4096)
    lib().pplan_schedule(rows, cols, int(use_orb), cfg.ctypes.data_as(C.c_void_p), names, values, len(env), out.ctypes.data_as(C.c_void_p), asked, 4096)
    return {f: int(out[i]) for i, f in enumerate(SCHEDULE_FIELDS)}, [n for n in asked.value.decode().split(";") if n]


def env_defaults():
    """the string orbfe_pipeline_env_defaults returns"""
    return lib().pplan_env_defaults().decode()
