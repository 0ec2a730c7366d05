"""Builds tests/detector_plan_driver.cpp (csrc/detector_plan.hpp behind a C ABI) with g++ and loads it with ctypes (test
infrastructure, in the manner of tests/extractor_plan_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build

_lib = None

SCALAR_FIELDS = ("win", "wpr", "npyr", "lds_bits_words", "relay_tbits", "relay_kshift", "relay_global", "relay_kcap", "ct_segcap", "ct_hbits",
                 "ct_lcap", "ct_items_per_frame")
SIZE_FIELDS = ("bits_fu32", "pyr_fbytes", "candq_fu32", "pool_fu32", "gpad_fu32")
MAXLEVELS = 16


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("detector_plan_driver.cpp", std="c++17", prefix="detector_plan_")
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_longlong
        L.dplan_make.argtypes = [i32, i32, i32, i32, i32, i32, i32, i64, vp, vp, vp, i32, vp, i32]
        L.dplan_threshold_sweep.argtypes = [i32, i32, i32, vp]
        L.dplan_input_layout.argtypes = [i32, i32, C.c_ulonglong, C.c_ulonglong, i32, vp, i32]
        L.dplan_pyramid_kernels.argtypes = [i32, i32, i32, i32, i32, i32, C.c_ulonglong, i32, vp, i32]
        L.dplan_switch_defaults.argtypes = [vp]
        L.dplan_read_env.argtypes = [vp, vp, i32, vp, vp, i32]
        L.dplan_batch.argtypes = [i32, i32, i32, i32, i32, i64, i32, i32, i32, i32, i32, vp, vp]
        L.dplan_escalate.argtypes = [i32, i32, i32]
        L.dplan_forced_speck_launch.argtypes = [i32, i32]
        L.dplan_threshold_predicate_differs.argtypes = [i32, i32]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def make(rows, cols, prows=None, pcols=None, S=35, specks_inkernel=0, lcap_override=0, rl_static=4352):
    """(error code, message, dict of scalars and sizes, levels as rows of (w, h, pitch, exact)) of the geometry.  S = 35: the ARUCO
    dictionary's warp size; rl_static: static LDS of the relay kernels, which the library asks of the runtime (4 KiB + 256 here)."""
    sc = np.zeros(len(SCALAR_FIELDS), np.int32); sz = np.zeros(len(SIZE_FIELDS), np.int64); lv = np.zeros((MAXLEVELS, 4), np.int32)
    msg = C.create_string_buffer(256)
    rc = lib().dplan_make(rows, cols, rows if prows is None else prows, cols if pcols is None else pcols, S, specks_inkernel, lcap_override,
                          rl_static, _p(sc), _p(sz), _p(lv), MAXLEVELS, msg, 256)
    d = {f: int(sc[i]) for i, f in enumerate(SCALAR_FIELDS)}
    d.update({f: int(sz[i]) for i, f in enumerate(SIZE_FIELDS)})
    return rc, msg.value.decode(), d, lv[:max(d["npyr"], 0)]


def mean_mismatches(n):
    """Box sums 0 .. 255 n whose integer mean (plain and multiply-shift) is not rint(s * (1.0 / n))."""
    return lib().dplan_mean_mismatches(n)


def threshold_sweep(w_first, w_last, win):
    """(number of widths whose matrix-core threshold tables are refused or wrong, the first of them)."""
    bad = np.zeros(1, np.int32)
    return lib().dplan_threshold_sweep(w_first, w_last, win, _p(bad)), int(bad[0])


def threshold_refused(cols, win):
    return bool(lib().dplan_threshold_refused(cols, win))


def input_layout(rows, cols, step, frame_stride, nframes):
    """(error code, message) of plan_input_layout for a caller's device frames."""
    msg = C.create_string_buffer(256)
    rc = lib().dplan_input_layout(rows, cols, step, frame_stride, nframes, msg, 256)
    return rc, msg.value.decode()


def threshold_read_end(cols, win):
    """the byte column behind the last one k_threshold_mfma loads from a row of a `cols`-wide frame (-1: tables do not apply)"""
    return lib().dplan_threshold_read_end(cols, win)


PYR_KERNELS = ("none", "k_half_pyr<4>", "k_half_pyr<3>", "k_half_area4", "k_half_area", "k_resize_level")   # PyrKernel (detector_plan.hpp)


def pyramid_kernels(rows, cols, base_off, step, frame_stride, half_pyr=True, first=1, S=35):
    """The kernel that writes each pyramid level >= `first` (names, level 1 first) for frames at an aligned allocation + base_off."""
    out = np.zeros(MAXLEVELS, np.int32)
    n = lib().dplan_pyramid_kernels(rows, cols, S, first, base_off & 15, step, frame_stride, int(half_pyr), _p(out), MAXLEVELS)
    assert n >= 1, n
    return [PYR_KERNELS[v] for v in out[1:n]]


# DetectorSwitches (detector_plan.hpp), in the driver's order
SWITCH_FIELDS = ("tiled", "banded", "band_rows", "tile_w", "tpw", "lcap", "specks", "specks_inkernel", "relay_wide", "small_separate", "thr_mfma",
                 "thr_mfma_auto", "thr_pyr", "half_pyr", "force_legacy", "big_mode")
PLAN_FIELDS = ("thr", "thr_kk", "nfuse", "specks", "contours", "band", "band_rows", "tile_w", "tpw", "relay", "small_separate", "walker_hbm")
CONTOURS = ("tiled", "relay", "walker", "big", "none")       # enum class Contours
THR = ("fixed", "mfma", "pyr", "box")                        # enum class Thr
RELAY = ("relay", "relay8", "wide", "relay8g")               # enum class Relay


def switch_defaults():
    """DetectorSwitches as a handle has them with no ORBFE_ARUCO_* variable set."""
    out = np.zeros(len(SWITCH_FIELDS), np.int32)
    lib().dplan_switch_defaults(_p(out))
    return {f: int(out[i]) for i, f in enumerate(SWITCH_FIELDS)}


def read_env(env):
    """(the switches read_detector_env leaves for the environment `env`, a dict -- the process environment is not touched --, the list
    of names it asked for)."""
    names = (C.c_char_p * max(len(env), 1))(*[k.encode() for k in env])
    values = (C.c_char_p * max(len(env), 1))(*[v.encode() for v in env.values()])
    out = np.zeros(len(SWITCH_FIELDS), np.int32)
    asked = C.create_string_buffer(4096)
    lib().dplan_read_env(names, values, len(env), _p(out), asked, 4096)
    return {f: int(out[i]) for i, f in enumerate(SWITCH_FIELDS)}, [n for n in asked.value.decode().split(";") if n]


def batch(rows, cols, B, floor="tiled", adaptive=True, thres_value=7, work=None, S=35, rl_static=4352, **switches):
    """plan_batch for B frames of rows x cols, as a dict with the enums by name.  work = (rows, cols) of a reduced working image under
    the frame's pyramid; keyword arguments override fields of the default DetectorSwitches."""
    sw = switch_defaults()
    assert set(switches) <= set(sw), switches
    sw.update(switches)
    swv = np.array([sw[f] for f in SWITCH_FIELDS], np.int32)
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    wr, wc = work if work else (rows, cols)
    rc = lib().dplan_batch(wr, wc, rows, cols, S, rl_static, B, int(adaptive), int(work is not None), thres_value, CONTOURS.index(floor), _p(swv), _p(out))
    assert rc == 0, rc
    d = {f: int(out[i]) for i, f in enumerate(PLAN_FIELDS)}
    d["thr"] = THR[d["thr"]]; d["contours"] = CONTOURS[d["contours"]]; d["relay"] = RELAY[d["relay"]]
    return d


def escalate(ran, flags_or, relay_ok):
    return CONTOURS[lib().dplan_escalate(CONTOURS.index(ran), flags_or, int(relay_ok))]


def threshold_predicate_differs(cols, win):
    return bool(lib().dplan_threshold_predicate_differs(cols, win))


def forced_speck_launch(cols, B):
    """whether plan_batch gives a `cols`-wide frame the speck launch when it is forced on"""
    return bool(lib().dplan_forced_speck_launch(cols, B))
