"""The marker detector's geometry plan (csrc/detector_plan.hpp), compiled with g++ and run without a GPU: the adaptive-threshold
window and the /2 pyramid against the oracle detector (which exposes both: its thresholded image is stage 0, its pyramid levels are
stages 1 .., so neither is restated here), every refusal with its error code, the sweep over all box sums that shows the threshold
kernels' integer mean to be the reference's rounded one, and the sweep that shows the matrix-core threshold tables valid for every
width and window they are asked for.  Then what decides what runs: the switches and their environment reader, plan_batch's
choice of kernels and paths by frame and batch size (every path is bit-exact, so only these tests notice a rule that moved), and
the retry ladder."""
import numpy as np
import pytest

import detector_plan_build as dp

ORBFE_ERR_INVALID = -1   # include/orbfe.h

GEOMETRIES = [
    # (rows, cols, minMarkerSize)
    (480, 640, 0.0),       # the bench geometries
    (720, 1280, 0.0),
    (1080, 1920, 0.0),
    (641, 427, 0.0),       # odd width, inexact levels
    (130, 96, 0.0),
    (64, 64, 0.0),         # no level below the frame itself
    (619, 1582, 0.0),      # partial tiles; the bit image only just fits LDS next to the relay kernels' tables
    (200, 2200, 0.0),      # above 2048 columns: window 17
    (480, 640, 0.1),       # minMarkerSize: a reduced working image under the full frame's pyramid
    (1080, 1920, 0.06),
]


def _frame(rows, cols, seed):
    """Ramps and noise: every window gives another thresholded image."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    return ((xx * 3 + yy * 5) % 200 + rng.integers(0, 56, (rows, cols))).astype(np.uint8)


@pytest.mark.parametrize("rows,cols,min_size", GEOMETRIES)
def test_geometry_against_the_oracle(oracle, rows, cols, min_size):
    img = _frame(rows, cols, rows + cols)
    ora = oracle.ArucoOracle("ARUCO")
    ora.set_detection_mode(0, min_size)
    ora.detect(img)
    wr, wc = ora.state()["work_shape"]
    assert (min_size > 0) == ((wr, wc) != (rows, cols))
    rc, msg, g, lv = dp.make(wr, wc, rows, cols)
    assert rc == 0, msg
    # the window: the one whose adaptive threshold of the working image is the oracle detector's thresholded image
    work = img if (wr, wc) == (rows, cols) else oracle.resize_nearest(img, wc, wr)
    thres = ora.stage_image(0)
    assert thres.shape == (wr, wc)
    assert [w for w in range(3, 32, 2) if np.array_equal(oracle.adaptive_threshold(work, w), thres)] == [g["win"]]
    # the pyramid: the oracle's levels, from the full frame
    assert g["npyr"] == ora.stage_count(2) == len(lv)
    for l in range(g["npyr"]):
        assert ora.stage_image(1 + l).shape == (lv[l][1], lv[l][0]), l
        if l:
            assert lv[l][3] == int(lv[l - 1][0] == 2 * lv[l][0] and lv[l - 1][1] == 2 * lv[l][1]), l
            assert lv[l][2] % 64 == 0 and lv[l][2] >= lv[l][0], l
    # the bit image and the per-frame blocks
    assert g["wpr"] == (wc + 31) // 32 and g["bits_fu32"] == g["wpr"] * wr
    padded = ((wc + 2 + 31) // 32) * (wr + 2) + 2
    assert g["gpad_fu32"] == padded and g["lds_bits_words"] in (0, padded)
    assert g["candq_fu32"] % 64 == 0 and g["candq_fu32"] >= wr * wc // 16 + 64
    assert g["pool_fu32"] >= 256 * 4096
    # the relay kernels: a 4096- or 8192-slot table; the bit image in HBM only where it does not fit LDS with the smaller one
    assert g["relay_tbits"] in (12, 13) and g["relay_kshift"] == 5
    assert g["relay_kcap"] == (4096 if g["relay_global"] else 1024)
    assert g["ct_segcap"] <= 65535 and (1 << g["ct_hbits"]) >= 2 * g["ct_segcap"] and 0 < g["ct_lcap"] <= g["ct_segcap"]
    assert g["ct_items_per_frame"] >= 4096
    # the speck scratch is added to the queue only when asked for, and nothing else moves
    rc2, _, g2, lv2 = dp.make(wr, wc, rows, cols, specks_inkernel=1)
    assert rc2 == 0 and g2["candq_fu32"] > g["candq_fu32"] and np.array_equal(lv, lv2)
    assert {k: v for k, v in g2.items() if k != "candq_fu32"} == {k: v for k, v in g.items() if k != "candq_fu32"}


def test_the_relay_choice_follows_the_frame_size():
    """The bench geometries: 640 x 480 keeps its bit image and a 4096-slot table in LDS, 1280 x 720 takes 8192 slots, the bit image
    of 1920 x 1080 stays in HBM; the list-capacity override is clamped to the segment capacity."""
    small, mid, big = (dp.make(r, c)[2] for r, c in ((480, 640), (720, 1280), (1080, 1920)))
    assert (small["relay_tbits"], small["relay_global"], small["ct_lcap"]) == (12, 0, 4096) and small["lds_bits_words"] > 0
    assert (mid["relay_tbits"], mid["relay_global"], mid["ct_lcap"]) == (13, 0, 16384) and mid["lds_bits_words"] > 0
    assert (big["relay_tbits"], big["relay_global"], big["relay_kcap"]) == (13, 1, 4096) and big["lds_bits_words"] == 0
    assert dp.make(480, 640, lcap_override=1000)[2]["ct_lcap"] == 1000
    assert dp.make(480, 640, lcap_override=1 << 20)[2]["ct_lcap"] == small["ct_segcap"]
    # 1582 x 619 with the 8192-slot table: 156,976 B of dynamic LDS, so up to 160 KiB - 156,976 = 6864 B of static LDS next to it;
    # one byte more and the frame takes the 4096-slot table, and with no room at all the relay kernels cannot run
    assert [dp.make(619, 1582, rl_static=s)[2]["relay_tbits"] for s in (6864, 6865, 160 * 1024)] == [13, 12, 0]


@pytest.mark.parametrize("rows,cols,code,what", [
    (480, 8001, ORBFE_ERR_INVALID, "larger than 8000"),
    (8001, 640, ORBFE_ERR_INVALID, "larger than 8000"),
    (480, 4096, ORBFE_ERR_INVALID, "threshold window 33 too large"),   # 15 * 4096 / 1920 = 32, made odd
    (480, 8000, ORBFE_ERR_INVALID, "too large"),
])
def test_plan_refusals(rows, cols, code, what):
    rc, msg, _, _ = dp.make(rows, cols)
    assert rc == code and what in msg, (rc, msg)
    assert dp.make(480, 4095)[0] == 0   # window 31: the widest frame the plan admits


def test_the_integer_box_mean_is_the_rounded_mean():
    """For every odd window 3 .. 31 -- every window the plan admits -- and every box sum s = 0 .. 255 n, n = win^2: the threshold
    kernels' (s + n / 2) / n, also as the multiply-shift (s + n / 2) * ceil(2^32 / n) >> 32, equals the reference's
    rint(s * (1.0 / n)).  An even n has ties, which rint sends to the even neighbour: there the comparison fails."""
    for win in range(3, 32, 2):
        assert dp.mean_mismatches(win * win) == 0, win
    assert dp.mean_mismatches(16) > 0 and dp.mean_mismatches(36) > 0   # (the check is live)


@pytest.mark.parametrize("win", range(3, 16, 2))
def test_matrix_core_threshold_tables_fit_every_width(win):
    """Every width 48 .. 8000: the tables of k_threshold_mfma come out applicable and, for every output column, the pass-1 box matrix
    holds exactly the `win` taps folded by BORDER_REPLICATE (and the selection matrix the column itself)."""
    bad, first = dp.threshold_sweep(48, 8000, win)
    assert bad == 0, "first refused or wrong width: %d" % first


def test_matrix_core_threshold_tables_say_where_they_do_not_apply():
    assert dp.threshold_sweep(40, 47, 7)[0] == 8                       # (the check is live: below 48 pixels the strips do not fit)
    assert all(dp.threshold_refused(c, 5) for c in range(1, 48)) and not dp.threshold_refused(48, 5)
    assert all(dp.threshold_refused(2200, w) for w in range(17, 32, 2)) and not dp.threshold_refused(2200, 15)


# ---- the switches, their environment reader, the batch plan and the retry ladder.  The expected values are literals: the rules as
# ---- the library has them, not recomputed here.

SWITCH_DEFAULTS = dict(tiled=-1, banded=-1, band_rows=0, tile_w=0, tpw=0, lcap=0, specks=-1, specks_inkernel=0, relay_wide=1, small_separate=-1,
                       thr_mfma=1, thr_mfma_auto=1, thr_pyr=1, half_pyr=1, force_legacy=0, big_mode=0)


def _pick(plan, *fields):
    return tuple(plan[f] for f in fields)


def test_switch_defaults():
    assert dp.switch_defaults() == SWITCH_DEFAULTS
    sw, asked = dp.read_env({})
    assert sw == SWITCH_DEFAULTS
    assert sorted(asked) == sorted("ORBFE_ARUCO_" + n for n in ("RELAY_WIDE", "SMALL_SEPARATE", "TILED", "BANDED", "BAND_ROWS", "TILE_W", "TPW", "LCAP", "SPECKS"))
    assert len(asked) == len(set(asked))   # each variable is looked up once


@pytest.mark.parametrize("var,cases", [
    # off only when set and atoi gives 0
    ("RELAY_WIDE", {"0": dict(relay_wide=0), "1": {}, "7": {}, "-1": {}, "": dict(relay_wide=0), "x": dict(relay_wide=0)}),
    # unset: by rule (-1); otherwise atoi != 0
    ("BANDED", {"0": dict(banded=0), "1": dict(banded=1), "5": dict(banded=1), "-3": dict(banded=1), "": dict(banded=0)}),
    ("TILED", {"0": dict(tiled=0), "1": dict(tiled=1), "5": dict(tiled=1), "-3": dict(tiled=1), "": dict(tiled=0)}),
    # unset: -1; otherwise atoi as it is
    ("SMALL_SEPARATE", {"0": dict(small_separate=0), "1": dict(small_separate=1), "9": dict(small_separate=9), "-2": dict(small_separate=-2)}),
    # unset: 0; otherwise atoi as it is (plan_batch and plan_detector take values <= 0 as "by rule")
    ("BAND_ROWS", {"0": {}, "1": dict(band_rows=1), "-4": dict(band_rows=-4), "100000": dict(band_rows=100000)}),
    ("TILE_W", {"0": {}, "1": dict(tile_w=1), "-4": dict(tile_w=-4), "100000": dict(tile_w=100000)}),
    ("TPW", {"0": {}, "1": dict(tpw=1), "-4": dict(tpw=-4), "100000": dict(tpw=100000)}),
    ("LCAP", {"0": {}, "1": dict(lcap=1), "-4": dict(lcap=-4), "100000": dict(lcap=100000)}),
    # unset: (-1, inside off); 1: the launch; 2: inside the relay kernels; anything else: neither
    ("SPECKS", {"0": dict(specks=0), "1": dict(specks=1), "2": dict(specks=0, specks_inkernel=1), "3": dict(specks=0), "-1": dict(specks=0)}),
])
def test_environment_reader(var, cases):
    """Every variable: unset (test_switch_defaults), "0", "1", values outside its range -- and it moves no field but its own."""
    for value, changed in cases.items():
        assert dp.read_env({"ORBFE_ARUCO_" + var: value})[0] == dict(SWITCH_DEFAULTS, **changed), (var, value)
    # a variable of the pipeline or a misspelt one is not the detector's
    assert dp.read_env({"ORBFE_" + var: "1", "ORBFE_ARUCO_" + var + "S": "1", "ORBFE_PHASE_PIN": "3"})[0] == SWITCH_DEFAULTS


def test_batch_plan_640x480():
    assert dp.make(480, 640)[2]["win"] == 5
    full = dp.batch(480, 640, 300)
    assert _pick(full, "thr", "nfuse", "contours", "relay") == ("mfma", 0, "relay", "relay")
    assert _pick(full, "specks", "small_separate", "walker_hbm") == (1, 0, 0)
    one = dp.batch(480, 640, 1)
    assert _pick(one, "thr", "thr_kk", "nfuse") == ("pyr", 163 | 163 << 16, 4)
    assert _pick(one, "contours", "band", "band_rows", "specks") == ("tiled", 1, 1, 0)
    one_relay = dp.batch(480, 640, 1, floor="relay")
    assert _pick(one_relay, "contours", "relay", "small_separate", "specks") == ("relay", "wide", 1, 0)
    # the thresholds of B
    assert [dp.batch(480, 640, B)["thr"] for B in (7, 8)] == ["pyr", "mfma"]
    assert [dp.batch(480, 640, B)["band"] for B in (4, 5, 16, 32, 33)] == [1, 0, 0, 0, 1]
    assert all(_pick(dp.batch(480, 640, B), "tile_w", "tpw") == (160, 1) for B in (5, 16))
    assert _pick(dp.batch(480, 640, 300), "tile_w", "tpw") == (320, 2)
    assert _pick(dp.batch(480, 640, 32), "contours", "specks") == ("tiled", 0)
    assert _pick(dp.batch(480, 640, 33), "contours", "specks") == ("relay", 1)
    assert [dp.batch(480, 640, B, floor="relay")["relay"] for B in (32, 33)] == ["wide", "relay"]
    assert [dp.batch(480, 640, B)["small_separate"] for B in (32, 33)] == [1, 0]


def test_batch_plan_1280x720():
    assert dp.make(720, 1280)[2]["win"] == 11
    p = dp.batch(720, 1280, 300)
    assert _pick(p, "thr", "contours", "band", "band_rows", "specks") == ("mfma", "tiled", 1, 6, 0)
    assert _pick(dp.batch(720, 1280, 300, banded=0), "band", "tile_w", "tpw") == (0, 448, 2)
    r = dp.batch(720, 1280, 300, floor="relay")
    assert _pick(r, "contours", "relay", "specks", "small_separate") == ("relay", "relay8", 1, 0)


def test_batch_plan_1920x1080():
    assert dp.make(1080, 1920)[2]["win"] == 15
    p = dp.batch(1080, 1920, 100)
    assert _pick(p, "thr", "contours", "band", "band_rows") == ("mfma", "tiled", 1, 4)
    r = dp.batch(1080, 1920, 100, floor="relay")
    assert _pick(r, "contours", "relay", "small_separate", "specks", "walker_hbm") == ("relay", "relay8g", 1, 0, 1)
    assert dp.batch(1080, 1920, 100, floor="relay", small_separate=0)["small_separate"] == 1   # always behind relay8g


def test_threshold_kernel_choice():
    assert dp.batch(480, 640, 1, adaptive=False)["thr"] == dp.batch(480, 640, 300, adaptive=False)["thr"] == "fixed"
    assert _pick(dp.batch(480, 640, 300, thr_mfma=0), "thr", "nfuse") == ("pyr", 4)            # "threshold_mfma" = 0
    assert dp.batch(480, 640, 300, thr_mfma=0, thr_pyr=0)["thr"] == dp.batch(480, 640, 1, thr_mfma=0, thr_pyr=0)["thr"] == "box"
    assert dp.batch(480, 640, 1, thr_mfma=1, thr_mfma_auto=0)["thr"] == "mfma"                 # "threshold_mfma" = 1
    assert dp.batch(480, 640, 1, thr_pyr=0)["thr"] == "mfma"
    # windows k_threshold_pyr is not built for; windows above 15
    assert dp.make(480, 1152)[2]["win"] == 9 and dp.make(200, 2200)[2]["win"] == 17
    assert dp.batch(480, 1152, 1)["thr"] == "mfma" and dp.batch(480, 1152, 1, thr_mfma=0)["thr"] == dp.batch(480, 1152, 300, thr_mfma=0)["thr"] == "box"
    assert dp.batch(200, 2200, 1)["thr"] == dp.batch(200, 2200, 300)["thr"] == "box"
    # a reduced working image (its pyramid starts from the full frame): the matrix-core kernel for one frame too, nothing fused
    assert dp.make(480, 640, 960, 1280)[2]["win"] == 5
    assert dp.batch(960, 1280, 1, work=(480, 640))["thr"] == "mfma"
    assert _pick(dp.batch(960, 1280, 1, work=(480, 640), thr_mfma=0), "thr", "nfuse") == ("pyr", 0)
    # n v + K must stay within 16 bits (window 15: ThresHold up to 36) and K must not be negative
    assert dp.batch(1080, 1920, 1, thres_value=36)["thr"] == "pyr"
    assert [dp.batch(1080, 1920, B, thres_value=37, thr_mfma=m)["thr"] for B in (1, 300) for m in (1, 0)] == ["mfma", "box", "mfma", "box"]
    for tv in (-1, -7):
        assert [dp.batch(480, 640, B, thres_value=tv, thr_mfma=m)["thr"] for B in (1, 300) for m in (1, 0)] == ["mfma", "box", "mfma", "box"], tv
    # (the matrix-core kernel's accumulators start at -K: |K| below 2^20, which no 8-bit ThresHold comes near)
    for tv in (-100000, 100000):
        assert [dp.batch(480, 640, B, thres_value=tv, thr_mfma=m)["thr"] for B in (1, 300) for m in (1, 0)] == ["box"] * 4, tv
    # the plan says "mfma" exactly where the tables come out applicable
    assert not any(dp.threshold_predicate_differs(c, w) for w in range(3, 32, 2) for c in list(range(1, 130)) + [640, 1280, 1920, 4095, 8000])


def test_forced_paths():
    for B in (1, 300):
        assert _pick(dp.batch(480, 640, B, big_mode=1), "contours", "walker_hbm") == ("big", 1)
        assert _pick(dp.batch(480, 640, B, floor="big"), "contours", "walker_hbm") == ("big", 1)
        assert _pick(dp.batch(480, 640, B, force_legacy=1), "contours", "walker_hbm") == ("walker", 0)
        assert _pick(dp.batch(480, 640, B, floor="walker"), "contours", "walker_hbm") == ("walker", 0)
    assert _pick(dp.batch(1080, 1920, 100, force_legacy=1), "contours", "walker_hbm") == ("walker", 1)
    assert dp.batch(480, 640, 1, tiled=0)["contours"] == "relay" and dp.batch(480, 640, 300, tiled=1)["contours"] == "tiled"
    assert dp.batch(720, 1280, 300, tiled=0)["contours"] == "relay"
    assert dp.batch(480, 640, 300, tiled=1, floor="relay")["contours"] == "relay"   # a retry is past the tiled path, forced or not
    # where the relay kernels cannot run (no room for their tables): tiled by rule, the single walker behind it
    assert dp.make(480, 640, rl_static=160 * 1024)[2]["relay_tbits"] == 0
    assert dp.batch(480, 640, 300, rl_static=160 * 1024)["contours"] == "tiled"
    assert dp.batch(480, 640, 300, rl_static=160 * 1024, floor="relay")["contours"] == "walker"


@pytest.mark.parametrize("env,args,field,want", [
    ({"ORBFE_ARUCO_SPECKS": "1"}, (480, 640, 1), "specks", 1),
    ({"ORBFE_ARUCO_SPECKS": "1"}, (720, 1280, 300), "specks", 1),
    ({"ORBFE_ARUCO_SPECKS": "2"}, (480, 640, 300), "specks", 0),
    ({"ORBFE_ARUCO_SMALL_SEPARATE": "0"}, (480, 640, 1), "small_separate", 0),
    ({"ORBFE_ARUCO_SMALL_SEPARATE": "1"}, (480, 640, 300), "small_separate", 1),
    ({"ORBFE_ARUCO_RELAY_WIDE": "0"}, (480, 640, 1), "relay", "relay"),
    ({"ORBFE_ARUCO_BAND_ROWS": "3"}, (720, 1280, 300), "band_rows", 3),
    ({"ORBFE_ARUCO_BAND_ROWS": "3"}, (480, 640, 1), "band_rows", 3),
    ({"ORBFE_ARUCO_TILE_W": "128"}, (480, 640, 300), "tile_w", 128),
    ({"ORBFE_ARUCO_TPW": "3"}, (480, 640, 300), "tpw", 3),
    ({"ORBFE_ARUCO_BANDED": "0"}, (480, 640, 300), "band", 0),
    ({"ORBFE_ARUCO_BANDED": "1"}, (480, 640, 16), "band", 1),
    ({"ORBFE_ARUCO_TILED": "1"}, (480, 640, 300), "contours", "tiled"),
])
def test_an_environment_switch_changes_the_field_it_names(env, args, field, want):
    """From the variable through read_detector_env to plan_batch: the named field moves to the forced value, the others stay (a forced
    path changes the speck launch with it: the launch's rule is about the path)."""
    base, forced = dp.batch(*args), dp.batch(*args, **dp.read_env(env)[0])
    assert base[field] != want and forced[field] == want
    moved = {f for f in dp.PLAN_FIELDS if base[f] != forced[f]}
    assert moved == ({field, "specks"} if field == "contours" else {field}), moved


def test_the_speck_launch_needs_its_tile_in_lds():
    """The launch's tile of 64 rows must fit 150 KB of LDS: up to 4766 columns.  Every frame the geometry admits (4095 columns) is
    narrower, so the plan's width check only ever refuses a geometry that plan_detector would not have made."""
    assert dp.make(480, 4095)[0] == 0 and dp.make(480, 8000)[0] == ORBFE_ERR_INVALID
    assert dp.batch(480, 4095, 1, specks=1)["specks"] == 1 and dp.batch(480, 4095, 300, specks=1)["specks"] == 1
    assert [dp.forced_speck_launch(c, B) for c in (640, 4095, 4766, 4767, 8000) for B in (1, 300)] == [True] * 6 + [False] * 4


CAPACITY_FLAGS, FALLBACK_FLAGS, TRUNCATED = (2, 4), (32, 64), 128


def test_the_retry_ladder():
    for relay_ok in (True, False):
        for ran in dp.CONTOURS[:4]:
            assert dp.escalate(ran, 0, relay_ok) == "none" and dp.escalate(ran, TRUNCATED, relay_ok) == "none", ran
        for f in CAPACITY_FLAGS + FALLBACK_FLAGS + (2 | 4 | 32 | 64 | 128,):
            assert dp.escalate("tiled", f, relay_ok) == ("relay" if relay_ok else "big"), f
            assert dp.escalate("big", f, relay_ok) == "none", f
        for f in CAPACITY_FLAGS + (2 | 4, 2 | 32, 4 | 64 | 128):
            assert dp.escalate("relay", f, relay_ok) == "big" and dp.escalate("walker", f, relay_ok) == "big", f
        for f in FALLBACK_FLAGS + (32 | 64, 32 | 64 | 128):
            assert dp.escalate("relay", f, relay_ok) == "none" and dp.escalate("walker", f, relay_ok) == "none", f
