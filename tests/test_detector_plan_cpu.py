"""The marker detector's geometry plan (csrc/detector_plan.hpp), compiled with g++ and run without a GPU: the adaptive-threshold
window and the /2 pyramid against the oracle detector (which exposes both: its thresholded image is stage 0, its pyramid levels are
stages 1 .., so neither is restated here), every refusal with its error code, the sweep over all box sums that shows the threshold
kernels' integer mean to be the reference's rounded one, and the sweep that shows the matrix-core threshold tables valid for every
width and window they are asked for."""
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
