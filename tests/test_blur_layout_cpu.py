"""The blurred pyramid's tiled layout (csrc/extractor_plan.hpp: 128-byte tiles, blur_tile_off / blur_pixel_off), without a GPU, on the
three bench geometries: the address function is injective over every level's pixels, levels do not overlap (one map of the frame's
block takes every pixel of every level: a byte claimed twice fails), every level is a whole number of line-aligned tiles and keeps to
them, a 16-byte chunk at a column that is a multiple of 16 is contiguous (k_orient_describe2 loads such chunks), and every pixel's
offset plus the largest read of that kernel -- one 16-byte chunk -- stays below blur_fbytes.  The same driver, built as a program of
its own with AddressSanitizer and UBSan, fills and de-tiles every level of the three geometries."""
import subprocess

import pytest

import blur_layout_build as bl

GEOMETRIES = [(480, 640, 1000, 8), (720, 1280, 2000, 8), (1080, 1920, 4000, 12)]   # rows, cols, nfeatures, nlevels (the bench's C2, C3, C5)
WHAT = {1: "plan refused", 2: "level not whole line-aligned tiles", 3: "two pixels share an offset", 4: "offset + over-read passes blur_fbytes",
        5: "a 16-byte chunk is not contiguous", 6: "a pixel leaves its level's tiles"}


def test_tile_is_one_line():
    tw, th = bl.tile_shape()
    assert tw * th == 128 and tw % 16 == 0


@pytest.mark.parametrize("rows,cols,nf,nl", GEOMETRIES)
def test_layout_is_injective_and_in_bounds(rows, cols, nf, nl):
    rc = bl.check(rows, cols, nf, nl)
    assert rc == 0, WHAT.get(rc, rc)


@pytest.mark.parametrize("rows,cols,nf,nl", GEOMETRIES + [(123, 161, 300, 4), (131, 175, 300, 4)])
def test_fill_and_detile_round_trip(rows, cols, nf, nl):
    assert bl.roundtrip(rows, cols, nf, nl) == 0


def test_fill_and_detile_under_sanitizers():
    exe = bl.sanitizer_program()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.count("check 0, 0 pixels differ") == 3, r.stdout
