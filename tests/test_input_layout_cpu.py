"""Which layouts of a caller's device frames the entry points admit (csrc/input_layout.hpp: plan_input_layout, carried by both plan
headers and compiled here with g++ through their test drivers), and the packing helper of the device-layout GPU tests
(tests/device_layouts.py).  No GPU.

The bounds are those of the kernels' offset arithmetic (input_layout.hpp derives them from the level-0 readers): a row step below 2^23
(24-bit multiplies), a frame span (rows - 1) * step + cols below 2^31 (32-bit sums), a frame stride that holds the span wherever a
second frame follows.  Each is checked at its last admitted and its first refused value."""
import numpy as np
import pytest

import detector_plan_build as dp
import device_layouts as dl
import extractor_plan_build as xp

ORBFE_ERR_INVALID = -1   # include/orbfe.h
DRIVERS = [pytest.param(xp.input_layout, id="extractor_plan"), pytest.param(dp.input_layout, id="detector_plan")]
STEP_END, SPAN_END = 1 << 23, 1 << 31


def _largest_step(rows, cols):
    """the largest step whose span (rows - 1) * step + cols stays below 2^31"""
    return (SPAN_END - 1 - cols) // (rows - 1)


ACCEPTED = [
    # (rows, cols, step, frame_stride, nframes)
    (240, 320, 320, 240 * 320, 8),                                   # tight
    (240, 320, 321, 240 * 321 + 3, 8),                               # odd step, a gap between frames
    (240, 320, 384, 239 * 384 + 320, 8),                             # the frame stride ends with the last row's pixels
    (240, 320, 320, 0, 1),                                           # one frame: the stride is not used
    (227, 321, 328, 227 * 328, 2),
    (2, 64, STEP_END - 1, 2 * (STEP_END - 1), 2),                    # the last admitted step
    (256, 64, STEP_END - 1, 256 * (STEP_END - 1), 2),                # span 255 * (2^23 - 1) + 64: below 2^31
    (480, 640, _largest_step(480, 640), 480 * _largest_step(480, 640), 2),   # the last admitted span at 480 rows
    (1, 4000, 4000, 4000, 3),                                        # one row: the span is cols
]

REFUSED = [
    (240, 320, 319, 240 * 320, 8, "less than the columns, 320"),
    (2, 64, STEP_END, 2 * STEP_END, 2, "24-bit"),                    # the first refused step
    (2, 64, STEP_END + 64, 2 * (STEP_END + 64), 2, "24-bit"),
    (480, 640, 1 << 40, 480 << 40, 1, "24-bit"),                     # (nothing wraps inside the check itself)
    (480, 640, _largest_step(480, 640) + 1, 480 * (_largest_step(480, 640) + 1), 2, "32-bit"),   # the first refused span at 480 rows
    (257, 640, STEP_END - 1, 257 * (STEP_END - 1), 2, "32-bit"),     # the last admitted step, but 256 * (2^23 - 1) + 640 = 2^31 + 384
    (4127, 4127, 1 << 20, 4127 << 20, 1, "32-bit"),                  # 4126 * 2^20 is 2^32 and more
    (240, 320, 384, 239 * 384 + 319, 2, "frame stride"),             # one byte short of the last row's pixels
    (240, 320, 320, 0, 2, "frame stride"),
    (0, 320, 320, 0, 1, "no frame"),
    (240, 0, 320, 0, 1, "no frame"),
    (240, 320, 320, 240 * 320, 0, "no frame"),
]


def test_the_span_cases_sit_on_the_bound():
    s = _largest_step(480, 640)
    assert 479 * s + 640 < SPAN_END <= 479 * (s + 1) + 640 and s < STEP_END
    assert 255 * (STEP_END - 1) + 64 < SPAN_END <= 256 * (STEP_END - 1) + 640


@pytest.mark.parametrize("layout", DRIVERS)
def test_admitted_layouts(layout):
    for rows, cols, step, fstride, n in ACCEPTED:
        rc, msg = layout(rows, cols, step, fstride, n)
        assert rc == 0 and msg == "", (rows, cols, step, fstride, n, rc, msg)


@pytest.mark.parametrize("layout", DRIVERS)
def test_refused_layouts(layout):
    for rows, cols, step, fstride, n, what in REFUSED:
        rc, msg = layout(rows, cols, step, fstride, n)
        assert rc == ORBFE_ERR_INVALID and what in msg, (rows, cols, step, fstride, n, rc, msg)


@pytest.mark.parametrize("layout", DRIVERS)
def test_every_test_layout_is_admitted(layout):
    """the layouts tests/test_device_layouts_gpu.py hands the entry points"""
    for rows, cols in ((240, 320), (232, 312), (222, 318), (227, 321), (128, 576), (128, 574)):
        for _, base, step, gap in dl.layouts(cols):
            assert layout(rows, cols, step, dl.frame_stride(rows, step, gap), 8) == (0, ""), (rows, cols, step, gap)


@pytest.mark.parametrize("fill", [0x00, 0xFF, dl.RANDOM])
@pytest.mark.parametrize("rows,cols,B", [(5, 7, 1), (6, 10, 3)])
def test_pack(rows, cols, B, fill):
    """The frames lie where the layout says -- through the helper's own view and through plain index arithmetic -- and every other
    byte, the 64 behind the last full step included, is the fill."""
    frames = np.random.default_rng(rows).integers(0, 256, (B, rows, cols), dtype=np.uint8)
    steps = set()
    for name, base, step, gap in dl.layouts(cols):
        steps.add(step % 8)
        buf = dl.pack(frames, base, step, gap, fill, seed=3)
        fs = rows * step + gap
        assert fs == dl.frame_stride(rows, step, gap)
        assert buf.dtype == np.uint8 and buf.shape == (base + (B - 1) * fs + rows * step + 64,), name
        assert np.array_equal(dl.view(buf, B, rows, cols, base, step, gap), frames), name
        is_pixel = np.zeros(buf.size, bool)
        for f in range(B):
            for y in range(rows):
                o = base + f * fs + y * step
                assert np.array_equal(buf[o:o + cols], frames[f, y]), (name, f, y)
                is_pixel[o:o + cols] = True
        assert is_pixel.sum() == frames.size                       # no two rows overlap
        assert np.array_equal(is_pixel, dl.pixel_mask(B, rows, cols, base, step, gap)), name
        if fill == dl.RANDOM:
            want = np.random.default_rng(3).integers(0, 256, buf.size, dtype=np.uint8)
            assert np.array_equal(buf[~is_pixel], want[~is_pixel]), name
            other = dl.pack(frames, base, step, gap, fill, seed=4)
            assert np.array_equal(other[is_pixel], buf[is_pixel]) and (step == cols and gap == 0 and base == 0 or not np.array_equal(other, buf))
        else:
            assert (buf[~is_pixel] == fill).all(), name
        assert (~is_pixel[-64:]).all()
    assert len(steps) >= 3                                          # the layouts differ in their row alignment


def test_the_layouts_are_what_they_are_named_for():
    for cols in (320, 312, 318, 321):
        lay = {n: (b, s, g) for n, b, s, g in dl.layouts(cols)}
        assert lay["tight"] == (0, cols, 0)
        assert lay["control"][1] % 64 == 0 and lay["control"][1] >= cols + 64
        b, s, g = lay["odd"]
        assert len({(b + y * s) % 16 for y in range(16)}) == (16 if cols % 2 == 0 else 8)   # the rows' residues mod 16 (an even step: every other one)
        b, s, g = lay["mod4"]
        assert b % 8 == 4 and (s - cols) == 4 and g == 4
        b, s, g = lay["mod8"]
        assert b % 16 == 8 and (s - cols) == 8 and g == 8
        b, s, g = lay["step8"]
        assert s % 8 == 0 and cols < s <= cols + 8 and (b, g) == (0, 0)


def test_planned_loads_of_level_0_end_with_the_row():
    """A tight layout is legal: a row of the caller's buffer may end with its last pixel (step == cols), so the 16-byte pieces the
    matrix-core kernels are told to load from level 0 -- planned on the host, clamped against cols -- must end at or before column
    cols, at every width: the GPU tests' own and every other the plans admit below 2048 (from there on the window is above 15 and k_threshold_mfma does not apply)."""
    for cols in [312, 318, 320, 321, 576] + list(range(62, 2048)):
        for ed in (0, 1):
            end = xp.level0_read_end(cols, ed)
            assert 16 <= end <= cols, (cols, ed, end)
        win = max(3, int(15 * float(cols) / 1920.)) | 1                    # the detector's window at this width
        end = dp.threshold_read_end(cols, win)
        assert 16 <= end <= cols, (cols, win, end)


# The detector's pyramid kernels by size and layout: the table of tests/test_device_layouts_gpu.py's docstring, written out level by
# level (level 1 first) -- from the kernels' own requirements (k_half_pyr<4> / <3>: 16- / 8-byte rows of 16 x 16 / 8 x 8 blocks and 5 / 4
# levels of exact halves; k_half_area4: 8-byte source rows; k_half_area: bytes; k_resize_level: inexact levels), not from the plan.
HP4, HP3, HA4, HA, RL = "k_half_pyr<4>", "k_half_pyr<3>", "k_half_area4", "k_half_area", "k_resize_level"
ALL = ("tight", "control", "odd", "mod4", "mod8", "step8")
PYRAMID_TABLE = {
    (240, 320): {**{n: [HP3, HP3, HP3] for n in ("tight", "control", "mod8", "step8")}, **{n: [HA, HA4, HA4] for n in ("odd", "mod4")}},
    (232, 312): {**{n: [HP3, HP3, HP3] for n in ("tight", "control", "mod8", "step8")}, **{n: [HA, HA4, HA4] for n in ("odd", "mod4")}},
    (222, 318): {**{n: [HA, RL, RL] for n in ("tight", "odd", "mod4", "mod8")}, **{n: [HA4, RL, RL] for n in ("control", "step8")}},
    (227, 321): {n: [RL, RL, HA4] for n in ALL},
    (128, 576): {**{n: [HP4, HP4, HP4, HP4] for n in ("tight", "control")}, **{n: [HP3, HP3, HP3, HA4] for n in ("mod8", "step8")},
                 **{n: [HA, HA4, HA4, HA4] for n in ("odd", "mod4")}},
    (128, 574): {**{n: [HA, RL, RL, RL] for n in ("tight", "odd", "mod4", "mod8")}, **{n: [HA4, RL, RL, RL] for n in ("control", "step8")}},
}


@pytest.mark.parametrize("rows,cols", sorted(PYRAMID_TABLE))
def test_pyramid_kernel_by_layout(rows, cols):
    """plan_pyramid_kernels (what the detector's pyramid() launches) against the table, for every layout and both settings of half_pyr
    (off: every k_half_pyr entry becomes k_half_area4), and behind k_threshold_pyr (first > 1: the caller's alignment no longer
    matters).  The misaligned layouts must never get a kernel that casts the caller's rows to uint2 / uint4; the aligned ones must not
    fall to the byte kernel."""
    for name, base, step, gap in dl.layouts(cols):
        fs = dl.frame_stride(rows, step, gap)
        want = PYRAMID_TABLE[(rows, cols)][name]
        assert dp.pyramid_kernels(rows, cols, base, step, fs, True) == want, (name, "half_pyr 1")
        assert dp.pyramid_kernels(rows, cols, base, step, fs, False) == [HA4 if k in (HP4, HP3) else k for k in want], (name, "half_pyr 0")
        if name in ("odd", "mod4"):
            assert dp.pyramid_kernels(rows, cols, base, step, fs, True)[0] in (HA, RL), name
        # from level 2 on the source is the detector's own block
        assert dp.pyramid_kernels(rows, cols, base, step, fs, True, first=2) == ["none"] + [HA4 if k in (HP4, HP3) else k for k in want[1:]], name
    # each alignment term on its own, at 128 x 576: base, step, frame stride
    assert dp.pyramid_kernels(128, 576, 0, 576, 128 * 576)[0] == HP4
    for base, step, fs, k in ((8, 576, 128 * 576, HP3), (0, 584, 128 * 584, HP3), (0, 576, 128 * 576 + 8, HP3),
                              (4, 576, 128 * 576, HA), (0, 580, 128 * 580, HA), (0, 576, 128 * 576 + 4, HA), (1, 576, 128 * 576, HA)):
        assert dp.pyramid_kernels(128, 576, base, step, fs)[0] == k, (base, step, fs)
