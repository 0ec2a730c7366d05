"""The pipeline's schedule plan (csrc/pipeline_plan.hpp), compiled with g++ and run without a GPU: the defaults by frame size, the
precedence of environment over configuration over default, the limits, the locks that turn the late describe off and what that does
to defer_post; and the list of ORBFE_* variables bench.py trusts, against the names the two environment readers really ask for."""
import re

import pytest

import detector_plan_build as dp
import pipeline_plan_build as pp

SIZES = [(480, 640), (720, 1280), (1080, 1920)]

# orbfe_pipeline_env_defaults() as the parent commit returned it
ENV_DEFAULTS = ("ORBFE_ENGINE_SETS=2;ORBFE_RECORD_SETS=4;ORBFE_PHASE_PIN=size;ORBFE_DET_PIN=4;ORBFE_DEFER_POST=size;ORBFE_DET_NOFORK=size;"
                "ORBFE_ARUCO_RELAY_WIDE=1;"
                "ORBFE_ARUCO_SPECKS=size;ORBFE_DESCRIBE_LATE=1;ORBFE_ARUCO_SMALL_SEPARATE=size;ORBFE_ARUCO_TILED=size;ORBFE_ARUCO_TILE_W=0;"
                "ORBFE_ARUCO_TPW=0;ORBFE_ARUCO_BANDED=size;ORBFE_ARUCO_BAND_ROWS=0;ORBFE_ARUCO_LCAP=0;"
                "ORBFE_GATHER_STREAM=0;ORBFE_RCCL_LIB=")


def S(rows, cols, use_orb=True, env=None, **config):
    return pp.schedule(rows, cols, use_orb, env, **config)[0]


@pytest.mark.parametrize("size,phase_pin,small", zip(SIZES, (2, 2, 1), (1, 0, 0)))
def test_size_defaults(size, phase_pin, small):
    s = S(*size)
    assert (s["D"], s["R"], s["det_pin"], s["gather_stream"]) == (2, 4, 4, 0)
    assert s["phase_pin"] == phase_pin and s["det_nofork"] == small
    # the late describe is on by default and turns defer_post on at every size; without it defer_post is the size default
    assert s["describe_late"] == 1 and s["defer_post"] == 1
    off = S(*size, env={"ORBFE_DESCRIBE_LATE": "0"})
    assert off["describe_late"] == 0 and off["defer_post"] == small
    assert {k: v for k, v in off.items() if k not in ("describe_late", "defer_post")} == {k: v for k, v in s.items() if k not in ("describe_late", "defer_post")}


def test_environment_beats_configuration_beats_default():
    late_off = {"ORBFE_DESCRIBE_LATE": "0"}   # (so that defer_post shows what was picked for it)
    for field, var, key, dflt, cfgv, envv in [("engine_sets", "ORBFE_ENGINE_SETS", "D", 2, 3, 5), ("record_sets", "ORBFE_RECORD_SETS", "R", 4, 3, 6),
                                              ("phase_pin", "ORBFE_PHASE_PIN", "phase_pin", 2, 0, 4), ("det_pin", "ORBFE_DET_PIN", "det_pin", 4, 0, 2),
                                              ("defer_post", "ORBFE_DEFER_POST", "defer_post", 1, 0, 1), ("det_nofork", "ORBFE_DET_NOFORK", "det_nofork", 1, 0, 1)]:
        assert S(480, 640, env=late_off)[key] == dflt, field
        assert S(480, 640, env=late_off, **{field: cfgv})[key] == cfgv, field
        assert S(480, 640, env=dict(late_off, **{var: str(envv)}), **{field: cfgv})[key] == envv, field
        assert S(480, 640, env=dict(late_off, **{var: str(envv)}))[key] == envv, field
        assert S(480, 640, env=dict(late_off, **{var: ""}), **{field: cfgv})[key] == cfgv, field     # an empty variable is not set
        assert S(480, 640, env=dict(late_off, **{var: ""}))[key] == dflt, field
    # the two variables without a configuration field
    assert S(480, 640, env={"ORBFE_GATHER_STREAM": "1"})["gather_stream"] == 1 and S(480, 640, env={"ORBFE_GATHER_STREAM": ""})["gather_stream"] == 0
    assert S(480, 640, env={"ORBFE_DESCRIBE_LATE": ""})["describe_late"] == 1
    # the environment's defer_post = 0 loses against the late describe as the configuration's does
    assert S(720, 1280, defer_post=0)["defer_post"] == 1 and S(720, 1280, env={"ORBFE_DEFER_POST": "0"})["defer_post"] == 1


def test_limits():
    assert S(480, 640, record_sets=1)["R"] == 2 and S(480, 640, env={"ORBFE_RECORD_SETS": "0"})["R"] == 2
    assert S(480, 640, engine_sets=0)["D"] == 1 and S(480, 640, env={"ORBFE_ENGINE_SETS": "-3"})["D"] == 1
    for size in SIZES:
        s = S(*size, use_orb=False, engine_sets=3)
        assert s["D"] == 1 and s["describe_late"] == 0 and s["defer_post"] == (1 if size == (480, 640) else 0)


@pytest.mark.parametrize("size,small", zip(SIZES, (1, 0, 0)))
def test_one_engine_set_has_no_late_describe(size, small):
    for s in (S(*size, env={"ORBFE_ENGINE_SETS": "1"}), S(*size, engine_sets=1)):
        assert s["D"] == 1 and s["describe_late"] == 0 and s["defer_post"] == small


def test_a_lock_on_stage_3_turns_the_late_describe_off():
    for pin in [3, 13] + list(range(30, 40)):
        s = S(720, 1280, phase_pin=pin)
        assert s["phase_pin"] == pin and s["describe_late"] == 0 and s["defer_post"] == 0, pin
        assert S(720, 1280, env={"ORBFE_PHASE_PIN": str(pin)})["describe_late"] == 0, pin
    for pin in (3, 13):
        s = S(720, 1280, det_pin=pin)
        assert s["det_pin"] == pin and s["describe_late"] == 0 and s["defer_post"] == 0, pin
        assert S(720, 1280, env={"ORBFE_DET_PIN": str(pin)})["describe_late"] == 0, pin
    # the other stages leave it on (det_pin's tens digit is no lock: 30 .. 39 only count for the extractor sets)
    for pin in (0, 1, 2, 4, 5, 12, 14, 21, 24, 40):
        assert S(720, 1280, phase_pin=pin)["describe_late"] == 1, pin
    for pin in (0, 1, 2, 4, 5, 12, 14, 30, 34):
        assert S(720, 1280, det_pin=pin)["describe_late"] == 1, pin


def test_the_environment_list_is_what_the_readers_ask_for():
    """bench.py marks a line as diagnostic by orbfe_pipeline_env_defaults(): every name either reader looks up is in it, every
    ORBFE_* name in it but ORBFE_RCCL_LIB is looked up by one of them, and the string is the parent's byte for byte."""
    text = pp.env_defaults()
    assert text == ENV_DEFAULTS
    listed = [kv.split("=", 1)[0] for kv in text.split(";") if kv]
    assert len(listed) == len(set(listed)) == 18 and all(re.fullmatch(r"ORBFE_[A-Z0-9_]+", n) for n in listed)
    asked = set(pp.schedule(480, 640)[1]) | set(dp.read_env({})[1])
    assert set(pp.schedule(480, 640, use_orb=False)[1]) <= asked
    assert asked <= set(listed), sorted(asked - set(listed))
    assert set(listed) - asked == {"ORBFE_RCCL_LIB"}
