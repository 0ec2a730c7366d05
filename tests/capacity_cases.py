"""Host-side builders of the cases the capacity contract of the two image engines is tested on (tests/test_capacity_contract_gpu.py),
and what the oracle says about them (tests/test_capacity_cases_cpu.py proves that they are not vacuous).  numpy, synth and the oracle
only: nothing here touches a GPU.

The batch is three 240 x 320 frames: scene A, a flat frame of grey 128 (no keypoint, no marker), scene B -- an empty frame between two
full ones, so that a frame which runs past its block lands in a block whose every slot must keep the sentinel.  Capacities are
derived from the oracle's counts (T_f keypoints, M_f markers of frame f), never written down."""
import functools

import numpy as np

import oracle_lib as oracle
from orb_slam2_aruco_amd import synth

ROWS, COLS = 240, 320
EXTRACTOR = (300, 1.2, 4, 20, 7)             # nfeatures, scale, levels, FAST thresholds: as in the device-layout tests
SEED_A, SEED_B = 30, 31
N_MARKERS, SIDE_RANGE = 5, (30, 60)
DICTIONARY = "ARUCO"
SENTINEL = 0xA5                              # fill of every output record before a call
CORNER_SUBPIX, CORNER_LINES, CORNER_NONE = 0, 1, 2
MARKER_SIZE = 0.187                          # Frame.cc:131
# TUM1.yaml of the reference rescaled from 1280 x 720 to the frame size is what the pipeline uses; the stand-alone pose calls take these
K4 = np.array([517.306408 * COLS / 1280, 516.469215 * ROWS / 720, 318.643040 * COLS / 1280, 255.313989 * ROWS / 720], np.float32)
DIST = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)


@functools.lru_cache(maxsize=None)
def frames():
    """(3, ROWS, COLS) uint8, read-only: scene A, flat, scene B"""
    a = synth.scene(ROWS, COLS, SEED_A, DICTIONARY, n_markers=N_MARKERS, side_range=SIDE_RANGE)[0]
    b = synth.scene(ROWS, COLS, SEED_B, DICTIONARY, n_markers=N_MARKERS, side_range=SIDE_RANGE)[0]
    f = np.stack([a, np.full((ROWS, COLS), 128, np.uint8), b])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def flat_frames():
    f = np.full((3, ROWS, COLS), 128, np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def keypoints():
    """the oracle's (keypoints, descriptors) of every frame, and per frame and level (level image, blurred image, quadtree keypoints).
    Like the reference, the oracle's extractor blurs only levels that hold keypoints; for the others the blurred image is the oracle's
    GaussianBlur(7 x 7, sigma 2) primitive on its own level image: the extractor under test blurs every level."""
    ora = oracle.OrbOracle(*EXTRACTOR)
    full, stages = [], []
    for img in frames():
        full.append(ora.extract(img))
        levels = []
        for l in range(EXTRACTOR[2]):
            plain, quad = ora.level_image(l), ora.level_keypoints(l, 1)
            levels.append((plain, ora.level_image(l, True) if len(quad) else blur7(plain), quad))
        stages.append(levels)
    return full, stages


def blur7(img):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros_like(img)
    oracle.lib().oracle_gaussian_blur7(img.ctypes.data, img.shape[1], img.shape[0], out.ctypes.data)
    return out


def totals():
    """T_f"""
    return [len(k) for k, _ in keypoints()[0]]


@functools.lru_cache(maxsize=None)
def markers(corner_method=CORNER_LINES):
    """the oracle's id-sorted marker list of every frame"""
    ora = oracle.ArucoOracle(DICTIONARY)
    ora.set_corner_method(corner_method)
    return [ora.detect(img) for img in frames()]


def marker_counts():
    """M_f"""
    return [len(m) for m in markers()]


def extractor_capacities():
    t = max(totals())
    return [1, 7, 64, t - 1, t, t + 1]


def detector_capacities():
    m = marker_counts()[0]
    return [1, m - 1, m, m + 1]
