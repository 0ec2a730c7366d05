"""Every scheduling option of the batched pipeline, and the reuse of an input buffer after orbfe_pipeline_input_done, against the
oracle (tests/pipeline_schedule_case.py runs the combinations of one frame size and one environment in a process of its own).

A schedule is the same kernels on the same inputs in another order, so its records must equal the oracle AND, byte for byte, the
default schedule's records of the same batches: a difference is a missing dependency between streams.  The byte comparison is stricter
than the oracle's tolerances on angles, corners and poses.  Each combination names the dependency it guards; a failure prints it."""
import functools
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# group -> (configuration of bench.CONFIGS, B, steps, ORBFE_* environment of the child, child timeout in seconds)
GROUPS = {
    "c2": ("C2", 12, 7, {}, 900),
    "c2_describe_late_0": ("C2", 12, 7, {"ORBFE_DESCRIBE_LATE": "0"}, 600),
    "c3": ("C3", 8, 5, {}, 900),
    "c3_describe_late_0": ("C3", 8, 5, {"ORBFE_DESCRIBE_LATE": "0"}, 600),
    "c5": ("C5", 4, 4, {}, 900),
    "host": ("C2", 96, 4, {}, 900),
}
# the combination every other one of its frame size is compared with, byte for byte
REFERENCE = {"C2": ("c2", "default"), "C3": ("c3", "default"), "C5": ("c5", "default")}

# a stage-3 lock turns the late describe off, which is not reported; at 640 x 480 defer_post is 1 either way, so only the 1280 x 720
# and 1920 x 1080 cases can see it (defer_post back at its size default, 0)
STAGE3_AT_VGA = "a stage-3 lock turns the late describe off (not visible at 640 x 480; the larger frame sizes check it)"
# (group, name, kind, pipeline keywords, expected effective schedule, what the combination guards)
COMBOS = [
    # ---- A1: 640 x 480
    ("c2", "default", "matrix", {}, {"D": 2, "R": 4, "phase_pin": 2, "det_pin": 4, "defer_post": 1, "det_nofork": 1},
     "the measured default: two extractor sets, late describe, deferred post-work"),
    ("c2", "engine_sets_1", "matrix", {"engine_sets": 1}, {"D": 1, "phase_pin": 0},
     "one extractor set: consecutive batches on one stream, no late describe"),
    ("c2", "engine_sets_3", "matrix", {"engine_sets": 3}, {"D": 3},
     "three extractor sets: the phase lock and the late describe across a ring of three"),
    ("c2", "record_sets_2", "matrix", {"record_sets": 2}, {"R": 2},
     "a record set rewritten every other step: the engines wait for the matching (and halo copy) of batch i - 2"),
    ("c2", "record_sets_3", "matrix", {"record_sets": 3}, {"R": 3},
     "engine set and record set out of phase (2 sets, 3 records): the wait for batch i - R crosses extractor streams"),
    ("c2", "record_sets_5", "matrix", {"record_sets": 5}, {"R": 5},
     "five record sets: the halo written into a set five steps after it was read"),
    ("c2", "phase_pin_0", "matrix", {"phase_pin": 0}, {"phase_pin": 0}, "extractor sets without a phase lock"),
    ("c2", "phase_pin_1", "matrix", {"phase_pin": 1}, {"phase_pin": 1}, "phase lock behind the other set's FAST"),
    ("c2", "phase_pin_3", "matrix", {"phase_pin": 3}, {"phase_pin": 3},
     "phase lock behind the other set's descriptors: " + STAGE3_AT_VGA),
    ("c2", "phase_pin_4", "matrix", {"phase_pin": 4}, {"phase_pin": 4}, "phase lock behind the other set's resize chain"),
    ("c2", "phase_pin_32", "matrix", {"phase_pin": 32}, {"phase_pin": 32},
     "two gates, the one in front of FAST on the descriptors: " + STAGE3_AT_VGA),
    ("c2", "det_pin_0", "matrix", {"det_pin": 0}, {"det_pin": 0}, "detector not gated on the extractor"),
    ("c2", "det_pin_1", "matrix", {"det_pin": 1}, {"det_pin": 1}, "detector behind the previous batch's FAST"),
    ("c2", "det_pin_2", "matrix", {"det_pin": 2}, {"det_pin": 2}, "detector behind the previous batch's quadtree"),
    ("c2", "det_pin_3", "matrix", {"det_pin": 3}, {"det_pin": 3},
     "detector behind the previous batch's descriptors: " + STAGE3_AT_VGA),
    ("c2", "det_pin_10", "matrix", {"det_pin": 10}, {"det_pin": 10}, "extractor enqueued first, detector ungated: a gate on stage 0 is no gate, not an invalid stage"),
    ("c2", "det_pin_12", "matrix", {"det_pin": 12}, {"det_pin": 12}, "detector behind this batch's quadtree"),
    ("c2", "det_pin_13", "matrix", {"det_pin": 13}, {"det_pin": 13},
     "detector behind this batch's descriptors: " + STAGE3_AT_VGA),
    ("c2", "det_pin_14", "matrix", {"det_pin": 14}, {"det_pin": 14}, "detector behind this batch's resize chain"),
    ("c2", "defer_post_0", "matrix", {"defer_post": 0}, {"defer_post": 1},
     "defer_post = 0 asked for: the late describe keeps the post-work deferred"),
    ("c2", "defer_post_0_engine_sets_1", "matrix", {"defer_post": 0, "engine_sets": 1}, {"D": 1, "defer_post": 0},
     "matching enqueued in the step itself, right behind the extractor's batch"),
    ("c2", "det_nofork_0", "matrix", {"det_nofork": 0}, {"det_nofork": 0}, "the detector's /2 pyramid on a forked stream"),
    ("c2", "use_aruco_0", "matrix", {"use_aruco": 0}, {}, "extractor and matching alone (keypoints, descriptors, matches)"),
    ("c2", "use_orb_0", "matrix", {"use_orb": 0}, {"D": 1}, "detector alone (markers and poses)"),
    # ---- A1: environment switches, one process per environment
    ("c2_describe_late_0", "describe_late_0", "matrix", {}, {"D": 2, "defer_post": 1},
     "ORBFE_DESCRIBE_LATE=0: each batch's descriptors in its own step"),
    ("c2_describe_late_0", "describe_late_0_defer_post_0", "matrix", {"defer_post": 0}, {"defer_post": 0},
     "ORBFE_DESCRIBE_LATE=0 and defer_post = 0: matching in the step, behind the whole extraction"),
    # ---- A2: larger frames, where the size-dependent defaults differ
    ("c3", "default", "matrix", {}, {"D": 2, "R": 4, "phase_pin": 2, "defer_post": 1, "det_nofork": 0},
     "1280 x 720 defaults: no forced det_nofork, late describe forcing the deferred post-work"),
    ("c3", "engine_sets_1", "matrix", {"engine_sets": 1}, {"D": 1, "defer_post": 0},
     "one extractor set: no late describe, post-work in the step (the 1280 x 720 default for it)"),
    ("c3", "defer_post_0_engine_sets_1", "matrix", {"defer_post": 0, "engine_sets": 1}, {"D": 1, "defer_post": 0},
     "post-work in the step behind a single extractor stream"),
    ("c3", "det_nofork_1", "matrix", {"det_nofork": 1}, {"det_nofork": 1}, "the detector's /2 pyramid in line"),
    ("c3", "det_pin_13", "matrix", {"det_pin": 13}, {"det_pin": 13, "defer_post": 0},
     "detector behind this batch's descriptors: a stage-3 lock turns the late describe off"),
    ("c3", "phase_pin_3", "matrix", {"phase_pin": 3}, {"phase_pin": 3, "defer_post": 0},
     "phase lock behind the other set's descriptors: a stage-3 lock turns the late describe off"),
    ("c3_describe_late_0", "describe_late_0", "matrix", {}, {"D": 2, "defer_post": 0},
     "ORBFE_DESCRIBE_LATE=0 at 1280 x 720: descriptors and post-work in the step"),
    ("c5", "default", "matrix", {}, {"D": 2, "phase_pin": 1, "defer_post": 1},
     "1920 x 1080 defaults: phase lock behind FAST, the detector's tiled path"),
    ("c5", "phase_pin_2", "matrix", {"phase_pin": 2}, {"phase_pin": 2}, "phase lock behind the quadtree at 1920 x 1080"),
    ("c5", "phase_pin_3", "matrix", {"phase_pin": 3}, {"phase_pin": 3, "defer_post": 0},
     "phase lock behind the descriptors at 1920 x 1080: a stage-3 lock turns the late describe off"),
    ("c5", "engine_sets_1", "matrix", {"engine_sets": 1}, {"D": 1}, "one extractor set at 1920 x 1080"),
    # ---- A3: one device buffer reused after orbfe_pipeline_input_done
    ("c2", "reuse_device_default", "reuse_device", {}, {"D": 2, "R": 4},
     "input_done enqueues the batch's held-back descriptor kernel, which reads level 0 from the caller's frames, and waits for it"),
    ("c2", "reuse_device_engine_sets_1", "reuse_device", {"engine_sets": 1}, {"D": 1},
     "input_done waits for the extractor and the detector of the batch"),
    ("c2", "reuse_device_record_sets_2", "reuse_device", {"record_sets": 2}, {"R": 2},
     "input_done with two record sets (only the last two batches readable)"),
    ("c2", "reuse_device_use_orb_0", "reuse_device", {"use_orb": 0}, {},
     "input_done waits for the detector alone"),
    ("c2_describe_late_0", "reuse_device_describe_late_0", "reuse_device", {}, {"D": 2},
     "input_done without the late describe: the step's own ex_done"),
    # ---- A4: one page-locked host buffer reused after orbfe_pipeline_input_done
    ("host", "reuse_host_use_aruco_1", "reuse_host", {}, {},
     "input_done waits for the upload of the caller's host frames (through the detector and the extractor)"),
    ("host", "reuse_host_use_aruco_0", "reuse_host", {"use_aruco": 0}, {},
     "input_done waits for the upload through the extractor alone, whose held-back descriptors it enqueues"),
]


@functools.lru_cache(maxsize=None)
def _run_group(group):
    """One child process for the group's combinations: (returncode, summary dict or None, output tail)."""
    config, B, steps, env, timeout = GROUPS[group]
    spec = {"config": config, "B": B, "steps": steps,
            "combos": [{"name": n, "kind": k, "kw": kw} for g, n, k, kw, _, _ in COMBOS if g == group]}
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("ORBFE_") or k == "ORBFE_LIB"}
    child_env.update(env)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "pipeline_schedule_case.py"), json.dumps(spec)], capture_output=True,
                           text=True, timeout=timeout, env=child_env)
    except subprocess.TimeoutExpired as e:
        # returned, not raised: the cache keeps the failure, and no later test of the group starts the hung workload again
        out = lambda b: (b.decode(errors="replace") if isinstance(b, bytes) else b or "")
        return False, None, "group %s timed out after %g s\n%s%s" % (group, timeout, out(e.stdout)[-3000:], out(e.stderr)[-4000:])
    lines = r.stdout.strip().splitlines()
    try:
        summary = next((json.loads(l[len("summary "):]) for l in lines if l.startswith("summary ")), None)
    except ValueError:
        summary = None
    ok = r.returncode == 0 and lines and lines[-1].startswith("ok") and summary is not None
    return ok, summary, r.stdout[-3000:] + r.stderr[-4000:]


def _result(group, name):
    ok, summary, tail = _run_group(group)
    assert ok, "child process of group %s did not finish:\n%s" % (group, tail)
    return summary["combos"][name], summary


def _first_difference(got, want):
    """(batch, field) pairs both digests have, and the first one that differs (None)."""
    common = [(b, f) for b in sorted(want, key=int) if b in got for f in want[b] if f in got[b]]
    diff = next(((b, f) for b, f in common if got[b][f] != want[b][f]), None)
    return common, diff


def _check(group, name, expect, guards):
    res, summary = _result(group, name)
    print(json.dumps({"combination": name, "group": group, "env": res["env"], "schedule": res["schedule"], "seconds": res["seconds"],
                      "batches_checked": res.get("batches_checked"), "keypoints_checked": res.get("keypoints_checked"),
                      "markers_checked": res.get("markers_checked"), "pairs_checked": res.get("pairs_checked")}))
    assert res["error"] is None, "%s (guards: %s): %s" % (name, guards, res["error"])
    for k, v in expect.items():
        assert res["schedule"][k] == v, ("%s: effective %s" % (name, k), res["schedule"], expect)
    ref_group, ref_name = REFERENCE[summary["config"]] if group != "host" else ("host", "reuse_host_use_aruco_1")
    if (ref_group, ref_name) == (group, name):
        return
    ref, _ = _result(ref_group, ref_name)
    assert ref["error"] is None, "reference combination %s failed: %s" % (ref_name, ref["error"])
    common, diff = _first_difference(res["digests"], ref["digests"])
    assert common, "%s shares no batch with %s" % (name, ref_name)
    assert diff is None, "%s (guards: %s): batch %s, field %s differs from %s's bytes" % (name, guards, diff[0], diff[1], ref_name)


def _ids(kinds):
    return [pytest.param(g, n, e, d, id=g + ":" + n) for g, n, k, _, e, d in COMBOS if k in kinds]


@pytest.mark.gpu
@pytest.mark.parametrize("group,name,expect,guards", [p for p in _ids({"matrix"}) if GROUPS[p.values[0]][0] == "C2"])
def test_schedule_640x480(group, name, expect, guards):
    """A1: C2 parameters, B = 12, 7 steps on 7 different batches, every readable record set and the newest matches against the oracle
    and against the default schedule's bytes.  Guards the stream dependencies each option adds or moves: the phase lock of the
    extractor sets, the detector's gate, the late describe, the deferred post-work, the wait for batch i - R before a record set is
    written again, the halo copy."""
    _check(group, name, expect, guards)


@pytest.mark.gpu
@pytest.mark.parametrize("group,name,expect,guards", [p for p in _ids({"matrix"}) if GROUPS[p.values[0]][0] in ("C3", "C5")])
def test_schedule_larger_frames(group, name, expect, guards):
    """A2: 1280 x 720 (C3, B = 8, 5 steps) and 1920 x 1080 (C5, B = 4, 4 steps), where the size-dependent defaults differ (post-work
    in the step, the detector's pyramid forked, the phase lock behind FAST, the detector's tiled path).  Guards the same dependencies
    as the 640 x 480 matrix under those defaults."""
    _check(group, name, expect, guards)


@pytest.mark.gpu
@pytest.mark.parametrize("group,name,expect,guards", _ids({"reuse_device"}))
def test_input_buffer_reuse_device(group, name, expect, guards):
    """A3: one device buffer (row pitch = the default + 64 bytes), refilled with the next batch by a blocking upload after each
    step's orbfe_pipeline_input_done.  Guards input_done: it must not return before every kernel that reads the caller's frames has
    run -- including the descriptor kernel the late describe holds back to the next step, which reads pyramid level 0 straight from
    those frames."""
    _check(group, name, expect, guards)


@pytest.mark.gpu
@pytest.mark.parametrize("group,name,expect,guards", _ids({"reuse_host"}))
def test_input_buffer_reuse_host(group, name, expect, guards):
    """A4: one page-locked buffer of 96 frames, overwritten in place (last frame first; the copy engine reads from the front) after
    each step_host's orbfe_pipeline_input_done; every record set's host copy against the oracle.  Guards input_done in host mode: it
    releases the caller's buffer only when the upload is done.  Without the detector, the only event that follows the upload is the
    extractor's, whose late descriptors input_done must enqueue; when that is missing the overwrite races the copy, so such a
    regression makes this test fail very likely but not certainly."""
    _check(group, name, expect, guards)
