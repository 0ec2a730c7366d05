"""The extractor's geometry plan (csrc/extractor_plan.hpp), compiled with g++ and run without a GPU: level sizes and quotas against the
oracle, the cell grid and the quadtree roots against the reference's formulas restated in float32 (the oracle computes both inside
ComputeKeyPointsOctTree / DistributeOctTree and exposes neither), every refusal with its error code, and the sweep that shows the
matrix-core blur tables valid for every level width the plan admits."""
import numpy as np
import pytest

import extractor_plan_build as xp

ORBFE_ERR_INVALID, ORBFE_ERR_CAPACITY = -1, -4   # include/orbfe.h

GEOMETRIES = [
    # (rows, cols, nfeatures, nlevels, scale factor)
    (480, 640, 1000, 8, 1.2),      # the bench geometries
    (720, 1280, 2000, 8, 1.2),
    (1080, 1920, 4000, 12, 1.2),
    (360, 636, 700, 6, 1.2),       # odd width, levels that are no multiple of 4
    (196, 1641, 500, 5, 1.2),      # panorama: ten quadtree roots
    (222, 222, 300, 8, 1.2),       # level 7 is 62 x 62: the smallest level the cell grid allows
    (62, 62, 100, 1, 1.2),
    (4127, 4127, 1000, 2, 2.0),    # the largest side a packed keypoint can carry
    (487, 1013, 1500, 7, 1.37),
]


def _tables(oracle, nf, nl, sf):
    t = oracle.OrbOracle(nf, sf, nl, 20, 7).tables()
    return t["scale"], t["inv_scale"], t["per_level"]


@pytest.mark.parametrize("rows,cols,nf,nl,sf", GEOMETRIES)
def test_plan_geometry_against_the_oracle(oracle, rows, cols, nf, nl, sf):
    scale, inv, quota = _tables(oracle, nf, nl, sf)
    rc, msg, lv, sc = xp.make(rows, cols, scale, inv, quota)
    assert rc == 0, msg
    # level sizes: the oracle's pyramid of a flat frame (ORBextractor.cc:1112); quotas: its constructor's table (:435-446)
    ora = oracle.OrbOracle(nf, sf, nl, 20, 7)
    ora.extract(np.full((rows, cols), 128, np.uint8))
    for l in range(nl):
        assert ora.level_image(l).shape == (lv["h"][l], lv["w"][l]), l
    assert np.array_equal(lv["quota"], quota)
    # cell grid (:767-787) and quadtree roots (:543): the reference's float arithmetic
    f32 = np.float32
    for l in range(nl):
        width, height = f32(lv["w"][l] - 32), f32(lv["h"][l] - 32)   # maxBorder - minBorder = (w - 19 + 3) - 16
        ncols, nrows = int(width / f32(30)), int(height / f32(30))
        wcell, hcell = int(np.ceil(width / f32(ncols))), int(np.ceil(height / f32(nrows)))
        assert (lv["nCols"][l], lv["nRows"][l], lv["wCell"][l], lv["hCell"][l]) == (ncols, nrows, wcell, hcell), l
        active = sum(1 for i in range(nrows) if 16 + i * hcell < lv["h"][l] - 16 - 3) * sum(1 for j in range(ncols) if 16 + j * wcell < lv["w"][l] - 16 - 6)
        assert lv["ncells"][l] == active, l
        q = float(width / height)
        nini = int(np.floor(q + 0.5))                                 # std::round of a positive float
        assert lv["nIni"][l] == nini and 1 <= nini <= 16, l
        assert lv["out_cap"][l] >= max(quota[l] + 3, 4 * nini), l
        assert lv["blur_strips"][l] == (lv["w"][l] + 31) // 32, l
    assert sc["ncells_total"] == lv["ncells"].sum() and sc["out_total"] == lv["out_cap"].sum()
    assert sc["max_wcell"] == lv["wCell"].max() and sc["max_hcell"] == lv["hCell"].max() and sc["max_ini"] == lv["nIni"].max()
    assert sc["nodecap"] == lv["out_cap"].max() + 8 and sc["veccap"] >= sc["nodecap"] and sc["veccap"] & (sc["veccap"] - 1) == 0
    assert sc["veccap"] < 2 * sc["nodecap"] and 0 <= sc["keycap_lds"] <= 6144 and sc["keycap_lds"] % 64 == 0
    # the taps do not move the geometry
    rc2, _, lv2, sc2 = xp.make(rows, cols, scale, inv, quota, 1)
    assert rc2 == 0 and sc2 == sc and all(np.array_equal(lv[k], lv2[k]) for k in lv)


@pytest.mark.parametrize("rows,cols,nf,nl,sf,code,what", [
    (100, 100, 1000, 8, 1.2, ORBFE_ERR_INVALID, "too small"),          # level 3 is 58 x 58
    (61, 640, 500, 1, 1.2, ORBFE_ERR_INVALID, "too small"),
    (480, 61, 500, 1, 1.2, ORBFE_ERR_INVALID, "too small"),
    (480, 4128, 500, 1, 1.2, ORBFE_ERR_INVALID, "above 4127"),
    (4128, 640, 500, 1, 1.2, ORBFE_ERR_INVALID, "above 4127"),
    (100, 3000, 500, 2, 1.2, ORBFE_ERR_INVALID, "quadtree roots"),     # 2968 / 68: 44 roots
    (640, 100, 500, 2, 1.2, ORBFE_ERR_INVALID, "quadtree roots"),      # 68 / 608: no root
    (480, 640, 30000, 8, 1.2, ORBFE_ERR_CAPACITY, "LDS"),              # level 0's quota of some 6500 keypoints
])
def test_plan_refusals(oracle, rows, cols, nf, nl, sf, code, what):
    scale, inv, quota = _tables(oracle, nf, nl, sf)
    rc, msg, _, _ = xp.make(rows, cols, scale, inv, quota)
    assert rc == code and what in msg, (rc, msg)


def test_matrix_core_blur_tables_fit_every_admitted_width():
    """Every level width the plan admits (62 .. 4127), both tap sets, both row-length rules (level 0: the width; levels >= 1: the
    width rounded up to 64): the tables of k_blur7_mfma come out valid and hold the 7 taps folded by BORDER_REFLECT_101 for every
    output column.  There is no second blur kernel for a width they would refuse."""
    bad, first = xp.blur_sweep(62, 4127)
    assert bad == 0, "first refused (width, taps, row rule): %r" % (first,)
    assert xp.blur_sweep(40, 47)[0] == 8 * 4     # (the check is live: below 48 pixels the strips do not fit)
