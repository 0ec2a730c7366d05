"""The host-only plan of LocalBundleAdjustment (csrc/lba_plan.hpp, with the camera step csrc/ba_camera.hpp shares with the pose
optimizer), compiled with g++ and run without a GPU: every rule of the validation in the order the functions apply them, the scratch
and staging layouts, the launch schedule.  The literals are the rules of local_ba.hip as they stood before the header existed; the
scratch totals were recorded from that library's orbfe_lba_scratch_bytes.  The same driver, built as a program of its own with
AddressSanitizer and UBSan, writes every array of both layouts and runs the validation on arrays of exactly their lengths."""
import math
import subprocess

import numpy as np
import pytest

import lba_plan_build as lp

OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -4   # include/orbfe.h

SIZE_TUPLES = [(0, 0, 0, 0, 0), (1, 1, 1, 0, 0), (3, 40, 80, 1, 3), (3, 257, 514, 0, 0), (64, 70, 4480, 0, 0), (256, 12, 3072, 0, 0),
               (40, 3000, 42000, 2, 5)]


def test_constants():
    assert lp.constants() == {"LBA_MAXV": 64, "LBA_N": 384, "LBA_PT": 64, "LBA_MAX_LEVELS": 32, "LBA_EBLK": 45, "LBA_MBLK": 90, "LBA_SE3_BYTES": 64,
                              "LBA_SOLVE_LDS": 4096, "sizeof_ctl": 144, "sizeof_result": 36}


# ---- the host calls' validation

def problem():
    """2 keyframes (the first fixed), 2 points seen 2 and 1 times, 1 marker seen once; 2 pyramid levels"""
    return dict(Tcw=np.full((2, 12), 0.5), kf_fixed=[1, 0], x3Dw=np.ones((2, 3)), obs_offset=[0, 2, 3], obs_kf=[0, 1, 0], obs_xy=np.full((3, 2), 10.0),
                obs_octave=[0, 1, 0], Twm=np.full((1, 12), 0.25), marker_local=np.full((1, 12), 0.1), mobs_offset=[0, 1], mobs_kf=[0],
                mobs_corners=np.full((1, 8), 20.0))


N = (2, 2, 3, 1, 1)


def _without(key):
    return lambda p: p.update({key: None})


def _nan_in(key):
    def f(p):
        p[key] = np.array(p[key], np.float32)
        p[key].reshape(-1)[-1] = np.nan
    return f


def _set(key, value):
    return lambda p: p.update({key: value})


# (what, the sizes, the change to problem(), code, text of the message), in the order lba_check_host applies its rules
HOST_CASES = [
    ("valid", N, None, OK, ""),
    ("negative size", (-1, 2, 3, 1, 1), None, ERR_INVALID, "invalid argument"),
    ("no Tcw", N, _without("Tcw"), ERR_INVALID, "invalid argument"),
    ("no kf_fixed", N, _without("kf_fixed"), ERR_INVALID, "invalid argument"),
    ("no x3Dw", N, _without("x3Dw"), ERR_INVALID, "invalid argument"),
    ("no obs_offset", N, _without("obs_offset"), ERR_INVALID, "invalid argument"),
    ("no obs_kf", N, _without("obs_kf"), ERR_INVALID, "invalid argument"),
    ("no obs_xy", N, _without("obs_xy"), ERR_INVALID, "invalid argument"),
    ("no obs_octave", N, _without("obs_octave"), ERR_INVALID, "invalid argument"),
    ("observations without points", (2, 0, 3, 1, 1), None, ERR_INVALID, "invalid argument"),
    ("no Twm", N, _without("Twm"), ERR_INVALID, "invalid argument"),
    ("no marker_local", N, _without("marker_local"), ERR_INVALID, "invalid argument"),
    ("no mobs_offset", N, _without("mobs_offset"), ERR_INVALID, "invalid argument"),
    ("no mobs_kf", N, _without("mobs_kf"), ERR_INVALID, "invalid argument"),
    ("no mobs_corners", N, _without("mobs_corners"), ERR_INVALID, "invalid argument"),
    ("marker observations without markers", (2, 2, 3, 0, 1), None, ERR_INVALID, "invalid argument"),
    ("Tcw not finite", N, _nan_in("Tcw"), ERR_INVALID, "an input is not finite"),
    ("x3Dw not finite", N, _nan_in("x3Dw"), ERR_INVALID, "an input is not finite"),
    ("obs_xy not finite", N, _nan_in("obs_xy"), ERR_INVALID, "an input is not finite"),
    ("Twm not finite", N, _nan_in("Twm"), ERR_INVALID, "an input is not finite"),
    ("marker_local not finite", N, _nan_in("marker_local"), ERR_INVALID, "an input is not finite"),
    ("mobs_corners not finite", N, _nan_in("mobs_corners"), ERR_INVALID, "an input is not finite"),
    ("obs_offset starts at 1", N, _set("obs_offset", [1, 2, 3]), ERR_INVALID, "obs_offset does not span [0, nobs]"),
    ("obs_offset ends at 2", N, _set("obs_offset", [0, 2, 2]), ERR_INVALID, "obs_offset does not span [0, nobs]"),
    ("obs_offset decreases", N, _set("obs_offset", [0, 4, 3]), ERR_INVALID, "obs_offset decreases at point 1"),
    ("mobs_offset starts at 1", N, _set("mobs_offset", [1, 1]), ERR_INVALID, "mobs_offset does not span [0, nmobs]"),
    ("mobs_offset ends at 2", N, _set("mobs_offset", [0, 2]), ERR_INVALID, "mobs_offset does not span [0, nmobs]"),
    ("mobs_offset decreases", (2, 2, 3, 2, 1),
     lambda p: p.update(Twm=np.full((2, 12), 0.25), marker_local=np.full((2, 12), 0.1), mobs_offset=[0, 2, 1]), ERR_INVALID,
     "mobs_offset decreases at marker 1"),
    ("keyframe 2 of 2", N, _set("obs_kf", [0, 1, 2]), ERR_INVALID, "observation 2 names keyframe 2 of 2"),
    ("keyframe -1", N, _set("obs_kf", [-1, 1, 0]), ERR_INVALID, "observation 0 names keyframe -1 of 2"),
    ("octave 2 of 2", N, _set("obs_octave", [0, 1, 2]), ERR_INVALID, "observation 2 has octave 2, outside [0, 2)"),
    ("octave -1", N, _set("obs_octave", [-1, 1, 0]), ERR_INVALID, "observation 0 has octave -1"),
    ("marker observation's keyframe", N, _set("mobs_kf", [2]), ERR_INVALID, "marker observation 0 names keyframe 2 of 2"),
    ("a keyframe observes a point twice", N, _set("obs_kf", [1, 1, 0]), ERR_INVALID, "keyframe 1 observes point 0 twice"),
]


@pytest.mark.parametrize("what,n,change,code,text", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_host_validation(what, n, change, code, text):
    p = problem()
    if change:
        change(p)
    rc, msg = lp.check_host(n, p, nlevels=2, use_markers=1)
    assert rc == code and text in msg, (rc, msg)
    assert msg.startswith("call: ") or rc == OK


def _free_keyframes(nkf, nma):
    return dict(Tcw=np.full((nkf, 12), 0.5), kf_fixed=np.zeros(nkf, np.uint8), Twm=np.full((nma, 12), 0.25), marker_local=np.full((nma, 12), 0.1),
                mobs_offset=np.zeros(nma + 1, np.int32))


def test_free_pose_bound():
    """64 free keyframes and 1 marker: 65 vertices with the markers in use, 64 without"""
    p = _free_keyframes(64, 1)
    rc, msg = lp.check_host((64, 0, 0, 1, 0), p, 2, use_markers=1)
    assert rc == ERR_CAPACITY and "65 free pose vertices" in msg and "ORBFE_LBA_MAX_FREE_POSES = 64" in msg
    assert lp.check_host((64, 0, 0, 1, 0), p, 2, use_markers=0) == (OK, "")
    p["kf_fixed"][5] = 1
    assert lp.check_host((64, 0, 0, 1, 0), p, 2, use_markers=1) == (OK, "")


def test_observation_bound():
    def seen_by(k):
        return dict(Tcw=np.full((k, 12), 0.5), kf_fixed=np.ones(k, np.uint8), x3Dw=np.ones((1, 3)), obs_offset=[0, k], obs_kf=np.arange(k),
                    obs_xy=np.full((k, 2), 10.0), obs_octave=np.zeros(k, np.int32))
    rc, msg = lp.check_host((257, 1, 257, 0, 0), seen_by(257), 2, 0)
    assert rc == ERR_CAPACITY and "point 0 has 257 observations" in msg and "ORBFE_LBA_MAX_OBSERVATIONS = 256" in msg
    assert lp.check_host((256, 1, 256, 0, 0), seen_by(256), 2, 0) == (OK, "")


def test_an_empty_problem_is_valid():
    assert lp.check_host((0, 0, 0, 0, 0), {}, 2, 1) == (OK, "")


def test_size_bounds():
    assert lp.sizes_ok((32768, 32767, 0, 0, 0)) and not lp.sizes_ok((32768, 32768, 0, 0, 0))      # nkf * np against 2^30
    assert lp.sizes_ok((1, 1, 1, 1, (1 << 24) - 1)) and not lp.sizes_ok((1, 1, 1, 1, 1 << 24))     # nmobs against 2^24
    assert lp.sizes_ok((0, 0, 0, 0, 0))
    for i in range(5):
        n = [1, 1, 1, 1, 1]
        n[i] = -1
        assert not lp.sizes_ok(n)


# ---- the device call's checks

def _addresses(**change):
    a = {k: 0x10000 + 0x100 * i for i, k in enumerate(lp.DEVICE_ARGS)}
    a.update(change)
    return a


XY_FORM = dict(obs_feature=0, kps=0)                  # the observations as values
KPS_FORM = dict(obs_xy=0, obs_octave=0)               # as features of keypoint blocks


def test_device_call_arguments():
    need = lp.scratch_bytes(N)
    good = lambda **c: lp.check_device(N, _addresses(**c), 0, need)
    assert good(**XY_FORM) == (OK, "")
    for k in ("Tcw", "kf_fixed", "x3Dw", "obs_offset", "obs_kf", "obs_octave", "Twm", "marker_local", "mobs_offset", "mobs_kf", "mobs_corners", "erase",
              "res", "scratch"):
        assert good(**dict(XY_FORM, **{k: 0})) == (ERR_INVALID, "call: invalid argument"), k
    # the other form needs the feature indices, the keypoint blocks and their capacity, and no octaves
    assert lp.check_device(N, _addresses(**KPS_FORM), 100, need) == (OK, "")
    assert lp.check_device(N, _addresses(**KPS_FORM), 0, need)[0] == ERR_INVALID
    assert lp.check_device(N, _addresses(obs_feature=0, **KPS_FORM), 100, need)[0] == ERR_INVALID
    assert lp.check_device(N, _addresses(kps=0, **KPS_FORM), 100, need)[0] == ERR_INVALID
    # what has no elements may be absent
    assert lp.check_device((0, 0, 0, 0, 0), dict(res=0x100, scratch=0x200), 0, lp.scratch_bytes((0, 0, 0, 0, 0))) == (OK, "")
    assert lp.check_device((2, 0, 3, 1, 1), _addresses(**XY_FORM), 0, need)[0] == ERR_INVALID      # observations without points
    assert lp.check_device((2, 2, 3, 0, 1), _addresses(**XY_FORM), 0, need)[0] == ERR_INVALID      # marker observations without markers
    assert lp.check_device((2, 2, 3, 1, 1 << 24), _addresses(**XY_FORM), 0, need)[0] == ERR_INVALID


def test_device_call_scratch():
    need = lp.scratch_bytes(N)
    for shift in (1, 128, 255):
        assert lp.check_device(N, _addresses(scratch=0x20000 + shift, **XY_FORM), 0, need) == (ERR_INVALID, "call: invalid argument")
    assert lp.check_device(N, _addresses(scratch=0x20000 + 256, **XY_FORM), 0, need) == (OK, "")
    rc, msg = lp.check_device(N, _addresses(**XY_FORM), 0, need - 1)
    assert rc == ERR_CAPACITY and msg == "call: %d bytes of scratch, orbfe_lba_scratch_bytes asks for %d" % (need - 1, need)
    # a misaligned scratch is refused as an argument before its size is looked at
    assert lp.check_device(N, _addresses(scratch=0x20080, **XY_FORM), 0, 0)[0] == ERR_INVALID


# ---- the layouts

ZEROED = ["ctl", "xv", "xl", "e_chi2", "m_chi2", "e_level", "m_level"]
# orbfe_lba_scratch_bytes of the library before the layout moved into the header
SCRATCH_TOTALS = {(0, 0, 0, 0, 0): 1218816, (1, 1, 1, 0, 0): 1218816, (3, 40, 80, 1, 3): 1262592, (3, 257, 514, 0, 0): 1477376,
                  (64, 70, 4480, 0, 0): 3003904, (256, 12, 3072, 0, 0): 2462208, (40, 3000, 42000, 2, 5): 18745344,
                  (32768, 32767, 0, 0, 0): 4307500288, (1, 1, 1, 1, (1 << 24) - 1): 49082957312}


def _check_arrays(arrays, end):
    at = 0
    for name, off, length in arrays:   # 256-byte aligned, in declaration order, none reaching into the next
        assert off % 256 == 0 and off >= at and length > 0, name
        at = off + length
    assert at <= end


@pytest.mark.parametrize("n", SIZE_TUPLES)
def test_scratch_layout(n):
    arrays, x = lp.scratch(n)
    assert [a[0] for a in arrays] == list(lp.SCRATCH_ARRAYS)
    _check_arrays(arrays, x["end"])
    # what is zeroed at every call is the state, the updates, the chi2 caches and the level bytes, whole, and nothing else
    assert [name for name, off, _ in arrays if off < x["zero_end"]] == ZEROED
    assert arrays[6][1] + arrays[6][2] <= x["zero_end"] == arrays[7][1] and x["zero_end"] % 256 == 0
    assert x["tbl_bytes"] == max(n[0], 1) * max(n[1], 1) * 4
    assert dict((a[0], a[2]) for a in arrays)["tbl"] == x["tbl_bytes"]
    assert x["end"] == lp.scratch_bytes(n) == SCRATCH_TOTALS[tuple(n)]


def test_scratch_totals_at_the_size_bounds():
    for n in ((32768, 32767, 0, 0, 0), (1, 1, 1, 1, (1 << 24) - 1)):
        assert lp.scratch_bytes(n) == SCRATCH_TOTALS[n]


def test_scratch_prefix_of_a_small_problem():
    arrays, x = lp.scratch((3, 40, 80, 1, 3))
    assert [(a[0], a[1]) for a in arrays[:9]] == [("ctl", 0), ("xv", 256), ("xl", 3328), ("e_chi2", 4352), ("m_chi2", 5120), ("e_level", 5376),
                                                  ("m_level", 5632), ("pose0", 5888), ("pose1", 6144)]
    assert x["zero_end"] == 5888


def test_sizes_of_zero_give_one_element_each():
    zero, one = lp.scratch((0, 0, 0, 0, 0)), lp.scratch((1, 1, 1, 1, 1))
    # one marker observation is a workgroup of corner edges beside the one of the points: a second partial sum, in the same 256 bytes
    assert lp.scratch((1, 1, 1, 1, 0)) == zero and [a[:2] for a in one[0]] == [a[:2] for a in zero[0]] and one[1] == zero[1]
    assert [a[2] for a in zero[0][-3:]] == [8, 8, 8] and [a[2] for a in one[0][-3:]] == [16, 16, 16]
    assert lp.host_io((0, 0, 0, 0, 0)) == lp.host_io((1, 1, 1, 1, 1))


@pytest.mark.parametrize("n", SIZE_TUPLES)
def test_staging_layout(n):
    arrays, x = lp.host_io(n)
    assert [a[0] for a in arrays] == list(lp.IO_ARRAYS)
    _check_arrays(arrays, x["end"])
    off = {a[0]: a[1] for a in arrays}
    # everything in front of the erase bytes goes up, everything from the poses on comes down
    assert x["split"] == off["erase"] and x["down"] == off["T"] and off["mcor"] < off["T"] < off["X"] < off["M"] < off["erase"] < off["res"] < x["end"]


def test_staging_layout_of_a_small_problem():
    arrays, x = lp.host_io((3, 40, 80, 1, 3))
    assert [a[1] for a in arrays] == [0, 256, 512, 1024, 1792, 2304, 2560, 2816, 3072, 3328, 3584, 4096, 4352, 4608]
    assert x == dict(split=4352, down=3328, end=4864)


# ---- the schedule

FULL = 1 + (1 + 5 * 53) + (2 + 10 * 53) + 2


def test_launch_counts():
    assert FULL == 801
    for n in SIZE_TUPLES:
        for use in (0, 1):
            s = lp.schedule(n, use)
            assert (s["launches"], s["rounds"], s["maxit0"], s["maxit1"], s["trials"]) == (801, 2, 5, 10, 10)
            s = lp.schedule(n, use, inspect=True)
            assert (s["launches"], s["rounds"], s["maxit0"], s["trials"]) == (9, 1, 1, 1)


def test_schedule_of_the_timing_problem():
    n = (40, 3000, 42000, 2, 5)
    s = lp.schedule(n, 1, lds_limit=163840)
    assert (s["npb"], s["nb"], s["g_setup"], s["g_pass"], s["g_points"], s["g_edges"]) == (47, 48, 165, 48, 47, 165)
    assert (s["vmax"], s["lds_rows"], s["tri_bytes"]) == (42, 198, 198 * 199 // 2 * 8)
    s = lp.schedule(n, 0, lds_limit=163840)
    assert (s["npb"], s["nb"], s["g_pass"], s["g_edges"], s["vmax"], s["lds_rows"]) == (47, 47, 47, 165, 40, 198)


@pytest.mark.parametrize("n", SIZE_TUPLES + [(70, 64, 0, 3, 0), (2, 65, 0, 1, 16), (2, 128, 0, 1, 17)])
def test_grids(n):
    nkf, np_, nobs, nma, nmobs = n
    for use in (0, 1):
        s = lp.schedule(n, use)
        assert s["npb"] == math.ceil(np_ / 64) and s["nb"] == s["npb"] + (math.ceil(4 * nmobs / 64) if use else 0)
        assert s["vmax"] == min(max(nkf + (nma if use else 0), 1), 64)
        assert s["g_setup"] == max(math.ceil(max(nobs, np_, nkf + nma, nmobs) / 256), 1)
        assert s["g_pass"] == max(s["nb"], 1) and s["g_points"] == max(s["npb"], 1)
        assert s["g_edges"] == max(math.ceil((nobs + (4 * nmobs if use else 0)) / 256), 1)
        assert min(s[k] for k in ("g_setup", "g_pass", "g_points", "g_edges", "vmax")) >= 1


def test_rows_of_the_reduced_system_in_lds():
    """the largest multiple of 6 that is at most 6 vmax and whose packed triangle fits beside the kernel's own 4 KB"""
    full = (64, 1, 0, 0, 0)
    assert lp.schedule(full, 0, lds_limit=65536)["lds_rows"] == 120 and lp.schedule(full, 0, lds_limit=163840)["lds_rows"] == 198
    assert lp.schedule(full, 0, lds_limit=65536)["tri_bytes"] == 120 * 121 // 2 * 8
    assert lp.schedule((3, 1, 0, 0, 0), 0, lds_limit=65536)["lds_rows"] == 18 and lp.schedule((0, 0, 0, 0, 0), 1)["lds_rows"] == 6
    for limit in (4096, 4096 + 167, 4096 + 168, 65536, 163840, 1 << 20):
        for vmax in (1, 3, 20, 21, 33, 34, 64):
            rows = lp.schedule((vmax, 1, 0, 0, 0), 0, lds_limit=limit)["lds_rows"]
            fits = lambda r: r * (r + 1) // 2 * 8 + 4096 <= limit
            assert rows % 6 == 0 and 0 <= rows <= 6 * vmax and (rows == 0 or fits(rows)), (limit, vmax, rows)
            assert rows == 6 * vmax or not fits(rows + 6), (limit, vmax, rows)
    # the whole system of 64 vertices needs 384 * 385 / 2 * 8 + 4096 bytes
    assert lp.schedule(full, 0, lds_limit=595456)["lds_rows"] == 384 and lp.schedule(full, 0, lds_limit=595455)["lds_rows"] == 378


# ---- the camera and level-table step both optimizers share

K4 = [517.3, 516.5, 318.6, 255.3]


@pytest.mark.parametrize("name", ["orbfe_pose_optimization", "orbfe_local_bundle_adjustment"])
def test_camera_step(name):
    rc, msg, c = lp.camera(name, K4, [1.0, 0.69444, 0.48225], 3, 25.0)
    assert (rc, msg) == (OK, "")
    assert np.array_equal(c["K4"], np.array(K4, np.float32)) and c["marker_info"] == 25.0 and c["nlevels"] == 3
    assert np.array_equal(c["inv_sigma2"], np.array([1.0, 0.69444, 0.48225] + [0.0] * 29, np.float32))
    assert c["delta"] == float(np.float32(math.sqrt(5.991)))
    refused = lambda *a: lp.camera(name, *a)[:2]
    assert refused(None, [1.0], 1, 25.0) == (ERR_INVALID, name + ": invalid K4 / sigma table")
    assert refused(K4, None, 1, 25.0) == (ERR_INVALID, name + ": invalid K4 / sigma table")
    assert refused(K4, [1.0], 0, 25.0) == (ERR_INVALID, name + ": invalid K4 / sigma table")
    assert refused(K4, [1.0] * 33, 33, 25.0) == (ERR_INVALID, name + ": invalid K4 / sigma table")
    assert refused(K4, [1.0] * 32, 32, 25.0) == (OK, "")
    for i in range(4):
        bad = list(K4)
        bad[i] = float("inf")
        assert refused(bad, [1.0], 1, 25.0) == (ERR_INVALID, name + ": K is not finite")
    assert refused([0.0] + K4[1:], [1.0], 1, 25.0) == (ERR_INVALID, name + ": fx or fy is 0")
    assert refused([K4[0], 0.0] + K4[2:], [1.0], 1, 25.0) == (ERR_INVALID, name + ": fx or fy is 0")
    assert refused(K4, [1.0], 1, float("nan")) == (ERR_INVALID, name + ": marker_info is not finite")
    # the table's entries are taken as they are: refusing a non-finite one is the bundle adjustment's own rule, not the pose optimizer's
    assert refused(K4, [float("nan")], 1, 25.0) == (OK, "")


# ---- the same rules under the sanitizers

def test_plan_under_sanitizers():
    exe = lp.sanitizer_program()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "lba_plan: 407 checks ok" in r.stdout, r.stdout
