"""The blurred pyramid in 128-byte tiles (csrc/extractor_plan.hpp: blur_tile_off), end to end against the CPU oracle: k_blur7_mfma writes
the tiles, k_orient_describe2 reads a keypoint's window from them as tile-aligned 16-byte chunks, orbfe_extractor_debug_level_image
puts a level's tiles back in rows.  Batches of 3 frames (frame index > 0 exercises the frame stride), four levels, 300 features, at

    160 x 120   level widths 160 133 111 93     161 x 123   161 134 112 93     175 x 131   175 146 122 101

so that a level width falls on a tile boundary (160), one pixel above one (161) and more than half a tile above one (175, 111, 93):
the test checks that from debug_level_size and the tile's width.  For every frame and level the blurred level equals the oracle's, and
every frame's keypoints and descriptors equal the oracle's, bit for bit.

The seeds (1, 2, 3 at every size; synth.scene with two markers of 30 - 44 pixels) were chosen on the CPU so that at every size the
oracle's keypoints of levels >= 1 come within 20 pixels of each of the four borders -- the windows that reach a level's first and last
column and row of tiles -- and meet both cases of the window's width: three chunks a row, and four when (kx - 18) mod 16 >= 12.  Both
are asserted from the oracle's keypoints: a run that never met the four-chunk case fails.  One single-frame host-pointer call
(orbfe_extract) on a 161 x 123 frame asks for the same equality."""
import numpy as np
import pytest

import blur_layout_build as bl
from orb_slam2_aruco_amd import binding, synth

pytestmark = pytest.mark.gpu

SIZES = [(120, 160), (123, 161), (131, 175)]   # rows, cols
SEEDS = (1, 2, 3)
NFEATURES, NLEVELS = 300, 4
_cache = {}


def _frames(rows, cols):
    key = ("frames", rows, cols)
    if key not in _cache:
        f = np.stack([synth.scene(rows, cols, s, n_markers=2, side_range=(30, 44))[0] for s in SEEDS])
        f.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def _reference(oracle, rows, cols):
    """per frame: (keypoints, descriptors, blurred levels, level keypoints in level coordinates) of the oracle; computed once"""
    key = ("ref", rows, cols)
    if key not in _cache:
        ref = []
        for img in _frames(rows, cols):
            ora = oracle.OrbOracle(NFEATURES, 1.2, NLEVELS, 20, 7)
            kps, desc = ora.extract(img)
            ref.append((kps, desc, [ora.level_image(l, True) for l in range(NLEVELS)], [ora.level_keypoints(l, 1) for l in range(NLEVELS)]))
        _cache[key] = ref
    return _cache[key]


def _same_features(got, want):
    kps, desc = got
    okps, odesc = want
    assert len(kps) == len(okps) and len(kps) > 0
    for fld in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(kps[fld], okps[fld]), fld
    assert np.array_equal(desc, odesc)


def test_level_widths_fall_on_above_and_off_a_tile_boundary():
    tw, _ = bl.tile_shape()
    rem = set()
    for rows, cols in SIZES:
        ex = binding.ORBextractor(NFEATURES, 1.2, NLEVELS, 20, 7, device=0)
        ex.extract_batch(_frames(rows, cols)[:1])
        rem |= {w % tw for w, _ in ex.level_sizes()}
    assert 0 in rem and 1 in rem and any(r > tw // 2 for r in rem), sorted(rem)


@pytest.mark.parametrize("rows,cols", SIZES)
def test_seeds_reach_the_borders_and_both_window_widths(oracle, rows, cols):
    left = right = top = bottom = three = four = 0
    for _, _, levels, lkps in _reference(oracle, rows, cols):
        for l in range(1, NLEVELS):
            h, w = levels[l].shape
            x, y = np.rint(lkps[l]["x"]).astype(int), np.rint(lkps[l]["y"]).astype(int)
            left += int((x <= 20).sum()); right += int((w - 1 - x <= 20).sum())
            top += int((y <= 20).sum()); bottom += int((h - 1 - y <= 20).sum())
            m = (x - 18) % 16
            three += int((m < 12).sum()); four += int((m >= 12).sum())
    assert min(left, right, top, bottom) > 0, (left, right, top, bottom)
    assert three > 0 and four > 0, (three, four)


@pytest.mark.parametrize("rows,cols", SIZES)
def test_batch_equals_the_oracle(oracle, rows, cols):
    ref = _reference(oracle, rows, cols)
    ex = binding.ORBextractor(NFEATURES, 1.2, NLEVELS, 20, 7, device=0)
    got = ex.extract_batch(_frames(rows, cols))
    for f in range(len(SEEDS)):
        for l in range(NLEVELS):
            assert np.array_equal(ex.level_image(f, l, True), ref[f][2][l]), (f, l)
        _same_features(got[f], ref[f][:2])


def test_single_frame_host_pointer_call_equals_the_oracle(oracle):
    rows, cols = SIZES[1]
    ref = _reference(oracle, rows, cols)
    ex = binding.ORBextractor(NFEATURES, 1.2, NLEVELS, 20, 7, device=0)
    got = ex(_frames(rows, cols)[1])
    for l in range(NLEVELS):
        assert np.array_equal(ex.level_image(0, l, True), ref[1][2][l]), l
    _same_features(got, ref[1][:2])
