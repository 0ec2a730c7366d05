"""GPU: the engines' named test switches (orbfe_extractor_debug_control / orbfe_aruco_debug_control) reject what they do not know
and then change nothing; the kernel-time read-out takes no control codes."""
import pytest

from orb_slam2_aruco_amd import synth

pytestmark = pytest.mark.gpu

ORBFE_ERR_INVALID = -1   # include/orbfe.h


def test_debug_control_rejects_unknown_keys_and_values(orbfe):
    img, _ = synth.scene(240, 320, 7, n_markers=2, side_range=(40, 70))
    ex = orbfe.ORBextractor(500, 1.2, 4, 20, 7)
    det = orbfe.MarkerDetector("ARUCO")
    common = [(b"no_such_key", 0), (b"", 0), (b"Kernel_timing", 1), (b"kernel_timing", 2), (b"kernel_timing", -1)]
    cases = [
        (ex, ex.L.orbfe_extractor_debug_control, ex.L.orbfe_extractor_debug_kernel_times, ex,
         [(b"general_quadtree", 2), (b"pyramid_depth", -1), (b"pyramid_depth", 7), (b"tiled_contours", 1)]),
        (det, det.L.orbfe_aruco_debug_control, det.L.orbfe_aruco_debug_kernel_times, det.detect,
         [(b"legacy_contours", 2), (b"tiled_contours", -2), (b"tiled_contours", 2), (b"speck_passes", -1), (b"speck_passes_in_kernel", 2),
          (b"threshold_pyr", 2), (b"threshold_mfma", -2), (b"threshold_mfma", 2), (b"half_pyr", -1), (b"pyramid_depth", 1)]),
    ]
    for h, control, times, run, bad in cases:
        for key, value in common + bad:
            assert control(h.h, key, value) == ORBFE_ERR_INVALID, (type(h).__name__, key, value)
        assert control(h.h, None, 1) == ORBFE_ERR_INVALID
        for capacity in (1, 32, -32):   # with no buffer the read-out is an error, not a switch (1 used to turn timing on)
            assert times(h.h, None, capacity) == ORBFE_ERR_INVALID, (type(h).__name__, capacity)
        run(img)
        assert len(h.kernel_times_us()) == 0, type(h).__name__   # none of the rejected calls switched kernel timing on
        assert control(h.h, b"kernel_timing", 1) == 0
        run(img)
        assert len(h.kernel_times_us()) > 0, type(h).__name__
