"""The capacity contract of the two image engines on device batches (include/orbfe.h at orbfe_extract_batch_device /
orbfe_extractor_batch_status, orbfe_aruco_detect_batch_device / orbfe_aruco_batch_status, orbfe_pipeline_status): a frame with more
records than the caller's `capacity` is clamped to a PREFIX of its full result, writes nothing outside its first `capacity` slots, and
is reported by the status call; the call is then repeated with a sufficient capacity.

The batch (tests/capacity_cases.py) is scene A, a flat frame, scene B, so a frame that runs past its block lands in a block whose every
slot must keep the sentinel.  Expected values are the CPU oracle's; capacities are derived from its counts.  Every case runs on the null
stream, inputs in Dev and outputs in Out buffers (256 guard bytes either side, checked by every get()), unwritten records pre-filled
with 0xA5.

Extractor: (a) clamp and prefix at capacities 1, 7, 64, max(T) - 1, max(T), max(T) + 1, (b) the status value and its clearing,
(c) the sticky flag, (d) repeat on one handle, whose flat (key, level) lists grow and then stay, (e) the host-pointer calls' own flag.
Detector: (f) clamp and prefix for the three corner-refinement methods, (g) poses on the truncated output, (h) the status with
ORBFE_ARUCO_FLAG_TRUNCATED, (i) the pipeline's marker_capacity and its status over several steps."""
import ctypes as C
import os

import numpy as np
import pytest

import capacity_cases as cc
import oracle_lib as oracle
from orb_slam2_aruco_amd import binding as orbfe
from pose_opt_device import Dev, Out

pytestmark = pytest.mark.gpu

B = 3
S = cc.SENTINEL
KP, MK, PS = orbfe.KP_DTYPE, orbfe.MARKER_DTYPE, orbfe.POSE_DTYPE
TRUNCATED = orbfe.ARUCO_FLAG_TRUNCATED
CORNER_TOL = 1e-3                            # px: the project's bar for marker corners
POSE_RTOL, POSE_ATOL, POSE_ERR_TOL = 1e-5, 1e-6, 1e-3   # tests/test_pose_gpu.py


@pytest.fixture(scope="module")
def d_frames():
    """the batch on the device, tightly packed (step = cols), shared by the module and never written"""
    return Dev(cc.frames())


@pytest.fixture(scope="module")
def ex():
    return orbfe.ORBextractor(*cc.EXTRACTOR)


def sentinel(dtype, *shape):
    return Out(np.full(shape + (dtype.itemsize,), S, np.uint8))


def records(out, dtype):
    """an Out of sentinel(dtype, ...) as records (get() checks the guards)"""
    raw = out.get()
    return raw.view(dtype).reshape(raw.shape[:-1]), raw


# ---------------------------------------------------------------------------------------------------------------- extractor

def extract(ex, d_img, cap):
    """one device batch at `cap`: (n [B], keypoints [B][cap], raw keypoint bytes, descriptors [B][cap][32])"""
    d_kps, d_desc, d_n = sentinel(KP, B, cap), Out(np.full((B, cap, 32), S, np.uint8)), Out(np.full(B, -7, np.int32))
    ex.extract_batch_device(d_img.ptr, B, cc.ROWS * cc.COLS, cc.ROWS, cc.COLS, cc.COLS, d_kps.ptr, d_desc.ptr, cap, d_n.ptr, None)
    n = d_n.get()                                                          # (blocking: waits for the null stream)
    kps, raw = records(d_kps, KP)
    return n, kps, raw, d_desc.get()


def check_prefix(n, kps, raw, desc, cap, what):
    """n[f] = min(T_f, cap); the first n[f] records and rows are the oracle's first n[f], byte for byte; the rest keeps the sentinel"""
    full, _ = cc.keypoints()
    assert n.tolist() == [min(len(k), cap) for k, _ in full], (what, n)
    for f, (ok, od) in enumerate(full):
        m = n[f]
        assert kps[f, :m].tobytes() == ok[:m].tobytes(), (what, f)
        assert np.array_equal(desc[f, :m], od[:m]), (what, f)
        assert (raw[f, m:] == S).all() and (desc[f, m:] == S).all(), (what, f)


def check_stages(ex, what):
    """the stage read-backs of the last batch do not depend on the capacity: of every frame and level, the flat frame's included, the
    quadtree keypoints (whole records), the level image and the blurred level image are the oracle's"""
    _, stages = cc.keypoints()
    for f in range(B):
        for l, (plain, blur, quad) in enumerate(stages[f]):
            got = ex.level_keypoints(f, l, 1)
            assert len(got) == len(quad) and got.tobytes() == quad.tobytes(), (what, f, l)
            assert np.array_equal(ex.level_image(f, l), plain), (what, f, l)
            assert np.array_equal(ex.level_image(f, l, True), blur), (what, f, l)


def expected_overflow(cap):
    return max([t for t in cc.totals() if t > cap], default=0)


def test_host_pointer_batch_at_full_capacity_is_the_oracle(ex):
    full, _ = cc.keypoints()
    assert ex.capacity >= max(cc.totals()) + 1
    got = ex.extract_batch(cc.frames())
    for f, ((k, d), (ok, od)) in enumerate(zip(got, full)):
        assert k.tobytes() == ok.tobytes() and np.array_equal(d, od), f
    assert ex.batch_status() == 0


@pytest.mark.parametrize("which", range(6))
def test_extractor_clamp_prefix_and_status(ex, d_frames, which):
    """(a), (b): which = index into capacity_cases.extractor_capacities(): 1, 7, 64, max(T) - 1, max(T), max(T) + 1"""
    cap = cc.extractor_capacities()[which]
    assert ex.batch_status() == 0
    n, kps, raw, desc = extract(ex, d_frames, cap)
    check_prefix(n, kps, raw, desc, cap, cap)
    assert n[1] == 0
    check_stages(ex, cap)
    want = expected_overflow(cap)
    assert (want > 0) == (cap < max(cc.totals()))
    assert ex.batch_status() == want                                       # the largest total that did not fit; 0 when all fit
    assert ex.batch_status() == 0                                          # reading cleared it


def test_extractor_flag_is_sticky_until_read(ex, d_frames):
    """(c): a clamping batch, a fitting batch, one read: the first batch's total; the second batch is complete"""
    t = max(cc.totals())
    assert ex.batch_status() == 0
    extract(ex, d_frames, 64)
    n, kps, raw, desc = extract(ex, d_frames, t)
    check_prefix(n, kps, raw, desc, t, "fitting batch behind a clamped one")
    assert n.tolist() == cc.totals()
    assert ex.batch_status() == expected_overflow(64) == t
    assert ex.batch_status() == 0


def test_extractor_repeat_with_the_reported_capacity():
    """(d): on a handle of its own, whose flat lists start at 3 x 7 entries: clamp at 7, repeat at the reported overflow (the lists
    grow), then 7 again on lists that stayed large"""
    ex, d_img = orbfe.ORBextractor(*cc.EXTRACTOR), Dev(cc.frames())
    first = extract(ex, d_img, 7)
    check_prefix(*first, 7, "first call at 7")
    ovf = ex.batch_status()
    assert ovf == max(cc.totals())
    n, kps, raw, desc = extract(ex, d_img, ovf)
    check_prefix(n, kps, raw, desc, ovf, "repeat")
    assert n.tolist() == cc.totals()
    assert ex.batch_status() == 0
    again = extract(ex, d_img, 7)
    check_prefix(*again, 7, "7 again")
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    check_stages(ex, "7 again")
    assert ex.batch_status() == ovf
    assert ex.batch_status() == 0


def test_extractor_host_pointer_calls_keep_their_own_flag(ex, d_frames):
    """(e): orbfe_extract below the frame's total is ORBFE_ERR_CAPACITY and leaves nothing in orbfe_extractor_batch_status; at the
    total it is the oracle; an unread overflow of a device batch neither fails a fitting host call nor is cleared by it"""
    L = orbfe.load()
    img = np.ascontiguousarray(cc.frames()[0])
    (ok, od), t_a = cc.keypoints()[0][0], cc.totals()[0]

    def host(cap):
        kps, desc, n = np.zeros(cap, KP), np.full((cap, 32), S, np.uint8), C.c_int32(-7)
        rc = L.orbfe_extract(ex.h, img.ctypes.data_as(C.c_void_p), cc.ROWS, cc.COLS, cc.COLS, kps.ctypes.data_as(C.c_void_p),
                             desc.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        return rc, n.value, kps, desc

    assert ex.batch_status() == 0
    rc, n, _, _ = host(t_a - 1)
    assert rc == orbfe.ORBFE_ERR_CAPACITY, (rc, L.orbfe_last_error())
    assert ex.batch_status() == 0                                          # the host call's flag is not the device batches'
    rc, n, kps, desc = host(t_a)
    assert rc == 0 and n == t_a, (rc, n, L.orbfe_last_error())
    assert kps.tobytes() == ok.tobytes() and np.array_equal(desc, od)
    extract(ex, d_frames, 7)                                               # a device batch overflows and nobody reads the flag
    rc, n, kps, desc = host(t_a)
    assert rc == 0 and n == t_a, (rc, n, L.orbfe_last_error())
    assert kps.tobytes() == ok.tobytes() and np.array_equal(desc, od)
    assert ex.batch_status() == max(cc.totals())                           # still there for the caller of the device batch
    assert ex.batch_status() == 0


# ----------------------------------------------------------------------------------------------------------------- detector

METHODS = {"lines": cc.CORNER_LINES, "none": cc.CORNER_NONE, "subpix": cc.CORNER_SUBPIX}
_dets = {}


def detector(method):
    """one handle a corner-refinement method (CORNER_SUBPIX without minMarkerSize: cornerSubPix runs on the clamped records)"""
    if method not in _dets:
        det = orbfe.MarkerDetector(cc.DICTIONARY)
        det.setCornerRefinementMethod(METHODS[method])
        _dets[method] = det
    return _dets[method]


def detect(det, d_img, cap):
    """one device batch at `cap`: (n [B], marker records [B][cap], their raw bytes, the Out buffers (markers, n), the status)"""
    d_out, d_n = sentinel(MK, B, cap), Out(np.full(B, -7, np.int32))
    det.detect_batch_device(d_img.ptr, B, cc.ROWS * cc.COLS, cc.ROWS, cc.COLS, cc.COLS, d_out.ptr, cap, d_n.ptr, None)
    n = d_n.get()
    rec, raw = records(d_out, MK)
    return n, rec, raw, (d_out, d_n), det.batch_status()


_full = {}


def detect_full(method, d_img):
    """the same device call at capacity orbfe_aruco_max_markers(): complete, unflagged, and the oracle's list"""
    if method not in _full:
        det = detector(method)
        n, rec, raw, _, status = detect(det, d_img, det.capacity)
        want = cc.markers(METHODS[method])
        assert status == (0, 0)
        assert n.tolist() == [len(m) for m in want]
        for f, m in enumerate(want):
            assert np.array_equal(rec[f, :n[f]]["id"], m["id"]), (method, f)
            assert np.abs(rec[f, :n[f]]["corners"] - m["corners"]).max(initial=0) <= CORNER_TOL, (method, f)
            assert (raw[f, n[f]:] == S).all(), (method, f)
        _full[method] = (n.copy(), rec.copy())
    return _full[method]


def flagged_frames(cap):
    return sum(m > cap for m in cc.marker_counts())


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("method", list(METHODS))
def test_detector_clamp_and_prefix(d_frames, method, which):
    """(f): which = index into capacity_cases.detector_capacities(): 1, M_A - 1, M_A, M_A + 1"""
    cap = cc.detector_capacities()[which]
    full_n, full_rec = detect_full(method, d_frames)
    want = cc.markers(METHODS[method])
    n, rec, raw, _, _ = detect(detector(method), d_frames, cap)
    assert n.tolist() == [min(len(m), cap) for m in want], (cap, n)
    assert n[1] == 0
    for f, m in enumerate(want):
        k = n[f]
        assert np.array_equal(rec[f, :k]["id"], m["id"][:k]), (cap, f)                       # the first k of the id-sorted list
        assert np.abs(rec[f, :k]["corners"] - m["corners"][:k]).max(initial=0) <= CORNER_TOL, (cap, f)
        assert rec[f, :k].tobytes() == full_rec[f, :k].tobytes(), (cap, f)                  # and of the call that fits, bit for bit
        assert (raw[f, k:] == S).all(), (cap, f)


@pytest.mark.parametrize("which", range(4))
def test_detector_status_counts_the_truncated_frames(d_frames, which):
    """(h): the frames with more markers than `capacity`, and only those, are flagged, with ORBFE_ARUCO_FLAG_TRUNCATED alone"""
    cap = cc.detector_capacities()[which]
    det = detector("lines")
    *_, status = detect(det, d_frames, cap)
    k = flagged_frames(cap)
    assert status == (k, TRUNCATED if k else 0), (cap, status)
    assert det.batch_status() == status                                    # per frame, of the last batch: reading does not clear
    if cap >= max(cc.marker_counts()):
        assert status == (0, 0)
    *_, status = detect(det, d_frames, max(cc.marker_counts()))            # the repeat with enough records
    assert status == (0, 0)
    assert det.contour_retries() == 0


def pose_matches(got, corners, K4, dist):
    r1, t1, r2, t2, err = oracle.marker_pose(corners, cc.MARKER_SIZE, K4, dist)
    a, b = np.concatenate([r1, t1, r2, t2]), np.concatenate([r2, t2, r1, t1])
    g = np.concatenate([got["rvec"], got["tvec"], got["rvec2"], got["tvec2"]]).astype(np.float64)
    ok = np.allclose(g, a, rtol=POSE_RTOL, atol=POSE_ATOL) and np.allclose(got["err"], err, atol=POSE_ERR_TOL)
    if not ok and abs(float(err[0]) - float(err[1])) < POSE_ERR_TOL:       # the two IPPE solutions reproject equally well: either order
        ok = np.allclose(g, b, rtol=POSE_RTOL, atol=POSE_ATOL)
    return ok


def marker_poses(d_markers_ptr, d_n_ptr, cap):
    d_poses = sentinel(PS, B, cap)
    rc = orbfe.load().orbfe_marker_poses_batch_device(d_markers_ptr, d_n_ptr, cap, B, cc.MARKER_SIZE, cc.K4.ctypes.data_as(C.c_void_p),
                                                      cc.DIST.ctypes.data_as(C.c_void_p), len(cc.DIST), d_poses.ptr, None)
    assert rc == 0, orbfe.load().orbfe_last_error()
    return records(d_poses, PS)


@pytest.mark.parametrize("which", range(4))
def test_poses_of_a_truncated_batch(d_frames, which):
    """(g): orbfe_marker_poses_batch_device with the detector's d_n writes exactly the first n[f] slots"""
    cap = cc.detector_capacities()[which]
    n, rec, _, (d_out, d_n), _ = detect(detector("lines"), d_frames, cap)
    poses, raw = marker_poses(d_out.ptr, d_n.ptr, cap)
    assert n.tolist() == [min(m, cap) for m in cc.marker_counts()]
    for f in range(B):
        for j in range(n[f]):
            assert pose_matches(poses[f, j], rec[f, j]["corners"], cc.K4, cc.DIST), (cap, f, j)
        assert (raw[f, n[f]:] == S).all(), (cap, f)
    rec2, raw2 = records(d_out, MK)                                        # the marker records are inputs: unchanged, guards intact
    assert rec2.tobytes() == rec.tobytes() and np.array_equal(d_n.get(), n)


def test_poses_without_counts_fill_every_slot():
    """(g): d_n == NULL: all `capacity` slots of every frame (here every slot holds a marker of the oracle's)"""
    want = cc.markers()
    cap = min(len(want[0]), len(want[2]))
    mk = np.stack([want[0][:cap], want[2][:cap], want[0][:cap][::-1]])
    d_mk = Dev(mk)
    poses, raw = marker_poses(d_mk.ptr, None, cap)
    for f in range(B):
        for j in range(cap):
            assert pose_matches(poses[f, j], mk[f, j]["corners"], cc.K4, cc.DIST), (f, j)


# ----------------------------------------------------------------------------------------------------------------- pipeline

def make_pipeline(describe_late, marker_capacity):
    """a pipeline for the batch; ORBFE_DESCRIBE_LATE is read when the pipeline is created"""
    from orb_slam2_aruco_amd import pipeline
    before = os.environ.get("ORBFE_DESCRIBE_LATE")
    if describe_late is None:
        os.environ.pop("ORBFE_DESCRIBE_LATE", None)
    else:
        os.environ["ORBFE_DESCRIBE_LATE"] = describe_late
    try:
        return pipeline.FrontEndPipeline(B, cc.ROWS, cc.COLS, nfeatures=cc.EXTRACTOR[0], nlevels=cc.EXTRACTOR[2], dictionary=cc.DICTIONARY,
                                         marker_capacity=marker_capacity)
    finally:
        if before is None:
            os.environ.pop("ORBFE_DESCRIBE_LATE", None)
        else:
            os.environ["ORBFE_DESCRIBE_LATE"] = before


def check_pipeline_markers(pipe, rec, mcap):
    want = cc.markers()
    assert rec["nmk"].tolist() == [min(len(m), mcap) for m in want]
    for f, m in enumerate(want):
        k = int(rec["nmk"][f])
        assert np.array_equal(rec["markers"][f, :k]["id"], m["id"][:k]), f
        assert np.abs(rec["markers"][f, :k]["corners"] - m["corners"][:k]).max(initial=0) <= CORNER_TOL, f
        for j in range(k):
            assert pose_matches(rec["poses"][f, j], rec["markers"][f, j]["corners"], pipe.cam_K, pipe.cam_D), (f, j)


@pytest.mark.parametrize("describe_late", [None, "0"], ids=["default_schedule", "describe_late_0"])
def test_pipeline_marker_capacity(describe_late):
    """(i): marker_capacity 2 cuts A and B to their first two markers (with poses) and orbfe_pipeline_status says so; 8 is complete and
    silent; a truncation in one step is still reported by a status call after a later, clean step"""
    import pipeline_check
    assert min(cc.marker_counts()[0], cc.marker_counts()[2]) > 2 and max(cc.marker_counts()) <= 8
    pipe = make_pipeline(describe_late, 2)
    assert pipe.mcap == 2
    d_img, d_flat = pipe.upload(cc.frames()), pipe.upload(cc.flat_frames())
    rec = pipe.read_records(pipe.step(d_img))
    check_pipeline_markers(pipe, rec, 2)
    assert rec["n"].tolist() == cc.totals()                                # the keypoint side of the record set is complete
    st = pipe.status()
    assert st["aruco_flagged_frames"] == 2 and st["aruco_flags"] == TRUNCATED, st
    assert st["extractor_overflow"] == 0 and st["search_init_overflow"] == 0, st
    assert not any(pipe.status().values())                                 # read and cleared
    # warmup() reads the same status: a frame over marker_capacity is reported as an error, and is no reason for the big-frame kernel
    with pytest.raises(orbfe.OrbfeError, match="capacity exceeded"):
        pipe.warmup(d_img, 1)
    assert pipe.big_frames is False and not any(pipe.status().values())
    # two steps, one read: the truncating batch, then three flat frames
    pipe.reset_stream()
    pipe.step(d_img)
    flat = pipe.read_records(pipe.step(d_flat))
    assert flat["nmk"].tolist() == [0, 0, 0] and flat["n"].tolist() == [0, 0, 0]
    st = pipe.status()
    assert st["aruco_flagged_frames"] == 2 and st["aruco_flags"] == TRUNCATED, st
    assert pipe.det.batch_status() == (0, 0)                               # the detector's own call: the last batch alone
    assert not any(pipe.status().values())
    del pipe
    pipe = make_pipeline(describe_late, 8)
    d_img = pipe.upload(cc.frames())
    rec = pipe.read_records(pipe.step(d_img))
    assert not any(pipe.status().values())
    check_pipeline_markers(pipe, rec, 8)
    pipeline_check.check_against_oracle(oracle, cc.frames(), range(B), rec, pipe.read_matches(), cc.EXTRACTOR[0], cc.EXTRACTOR[2],
                                        cc.DICTIONARY, cc.COLS, cc.ROWS, pipe.cam_K, pipe.cam_D, pairs=range(B - 1))
