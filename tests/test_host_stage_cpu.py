"""The staging layout of the host-pointer solver calls (IoLayout, csrc/host_stage.hpp), compiled with g++ and run without a GPU:
every array starts on a 256-byte boundary, the arrays lie one behind the other without touching, and what is uploaded is not
what is downloaded."""
import pytest

import host_stage_build as hs

SIZES = [0, 1, 255, 256, 257, 0, 1000, 28 * 2000, 3, 256, 0]


def _check(sizes, offsets, begin, end):
    """the slices of `sizes` at `offsets` lie in [begin, end), in order, disjoint, each on a 256-byte boundary"""
    at = begin
    for size, off in zip(sizes, offsets):
        assert off % 256 == 0 and off >= at, (sizes, offsets)
        at = off + size
    assert at <= end and end % 256 == 0


@pytest.mark.parametrize("n_in", range(len(SIZES) + 1))
def test_slices_are_aligned_disjoint_and_in_order(n_in):
    ins, outs = SIZES[:n_in], SIZES[n_in:]
    i_off, o_off, up, down = hs.layout(ins, outs)
    assert up[0] == 0 and up[1] == down[0] and down[0] <= down[1]   # the two ranges share no byte
    _check(ins, i_off, *up)
    _check(outs, o_off, *down)
    # an array of no bytes takes no room, every other one its size rounded up
    assert down[1] == sum((s + 255) // 256 * 256 for s in SIZES)


def test_layout_of_zero_sizes_is_empty():
    i_off, o_off, up, down = hs.layout([0, 0, 0], [0, 0])
    assert i_off == [0, 0, 0] and o_off == [0, 0] and up == (0, 0) and down == (0, 0)
    assert hs.layout([], []) == ([], [], (0, 0), (0, 0))


@pytest.mark.parametrize("n_in,n_io", [(0, 0), (0, 3), (2, 0), (2, 1), (3, 4), (5, 6), (11, 0), (4, 7)])
def test_inout_arrays_lie_in_both_ranges(n_in, n_io):
    """[inputs][in-out][outputs]: the upload range ends behind the in-out arrays, the download range begins in front of them; the
    inputs are only uploaded, the outputs only downloaded, and the mark moves no array (the offsets are those of the plain layout)."""
    ins, ios, outs = SIZES[:n_in], SIZES[n_in:n_in + n_io], SIZES[n_in + n_io:]
    i_off, b_off, o_off, up, down = hs.layout3(ins, ios, outs)
    assert up[0] == 0 and down[0] <= up[1] <= down[1]
    _check(ins, i_off, 0, down[0])
    _check(ios, b_off, down[0], up[1])
    _check(outs, o_off, up[1], down[1])
    assert up[1] - down[0] == sum((s + 255) // 256 * 256 for s in ios)   # the shared bytes are the in-out arrays and nothing else
    plain = hs.layout(ins + ios, outs)
    assert (i_off + b_off, o_off, up) == plain[:3] and down[1] == plain[3][1]
