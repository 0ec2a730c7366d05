"""The cases of tests/capacity_cases.py are not vacuous: with the oracle alone, both scenes hold enough keypoints and markers for
every capacity of tests/test_capacity_contract_gpu.py to clamp a frame, their totals differ (so the status can tell which frame it
reports), and the flat frame between them holds nothing."""
import numpy as np

import capacity_cases as cc


def test_frames():
    f = cc.frames()
    assert f.shape == (3, cc.ROWS, cc.COLS) and f.dtype == np.uint8 and (f[1] == 128).all()
    assert not np.array_equal(f[0], f[2])


def test_keypoint_totals():
    t_a, t_flat, t_b = cc.totals()
    assert t_a >= 100 and t_b >= 100 and t_a != t_b and t_flat == 0
    caps = cc.extractor_capacities()
    assert caps == [1, 7, 64, max(t_a, t_b) - 1, max(t_a, t_b), max(t_a, t_b) + 1] and min(caps) >= 1
    # a clamped frame cuts the ascending-level concatenation: the oracle's octaves ascend, so "the first n records" is a cut of it
    for k, _ in cc.keypoints()[0]:
        assert np.all(np.diff(k["octave"]) >= 0)
    full, stages = cc.keypoints()
    for f in (0, 2):
        assert sum(len(q) for _, _, q in stages[f]) == len(full[f][0])
    for plain, blur, q in stages[1]:                                        # the flat frame: no keypoints, and a blur to compare with
        assert len(q) == 0 and plain.shape == blur.shape and blur.min() == blur.max() and abs(int(blur[0, 0]) - 128) <= 1


def test_marker_counts():
    m_a, m_flat, m_b = cc.marker_counts()
    assert m_a >= 4 and m_b >= 3 and m_flat == 0
    caps = cc.detector_capacities()
    assert caps == [1, m_a - 1, m_a, m_a + 1] and min(caps) >= 1 and len(set(caps)) == 4
    for method in (cc.CORNER_SUBPIX, cc.CORNER_LINES, cc.CORNER_NONE):
        got = cc.markers(method)
        assert [len(m) for m in got] == [m_a, 0, m_b], method
        for m in got:                                                       # id order, one record an id: a prefix is defined
            assert np.all(np.diff(m["id"]) > 0)
