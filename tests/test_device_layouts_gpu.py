"""The device-pointer entry points on the layouts a caller's buffer may have: orbfe_extract_batch_device and
orbfe_aruco_detect_batch_device read pyramid level 0 straight from the caller's frames (ImgView{base, fstride, pitch}), so the base
may sit at any byte, the row step may be any value >= cols, frames may lie further apart than rows * step, and the bytes that are no
pixels hold anything.  The host-pointer entry points re-stage every frame into 64-byte rows at an aligned base and never see any of
that; they are the reference here: every device call must equal the host-pointer call on the same frames BIT FOR BIT (the same
kernels on the same pixels: no tolerance), for both of two fills of the slack, and must leave the caller's buffer as it was.

Layouts (tests/device_layouts.py: name, base offset, step, gap between frames), each with fills (0x00 | 0xFF by layout, random bytes):
  tight (0, cols, 0)    control (0, align64(cols) + 64, 0)    odd (1, cols + 1, 3)    mod4 (4, cols + 4, 4)    mod8 (8, cols + 8, 8)
  step8 (0, the next multiple of 8 above cols, 0)
Sizes (rows x cols), B = 2 and B = 8 frames of synth.scene with two markers; extractor: 300 features, 4 levels, scale 1.2.
  240 x 320, 232 x 312, 222 x 318, 227 x 321: extractor and detector.  128 x 576 and 128 x 574: detector only -- see below.

Which kernel reads the caller's rows, from the plans (extractor_plan.hpp / orb_extractor.hip plan_batch; detector_plan.hpp /
aruco_detector.hip plan_batch, pyramid(), work_size):
  Extractor, every size and layout: k_resize_tab (level 1 from level 0; resize_tab_ok holds at scale 1.2, so the extractor's
  k_resize_level is not reached), k_blur7_mfma (level 0's strips, pieces clamped against cols), k_fast_cells (ROI staging),
  k_orient_describe2 (patch rows of level-0 keypoints).
  Detector threshold.  The window is 3 below 512 columns, 5 at 576.  k_threshold_pyr exists for windows 5, 7, 11 and 15 only, so it is
  reached at the 128-row sizes alone; and only they give the detector 5 pyramid levels, which k_half_pyr<4> needs (320 columns give 4: 320,
  160, 80, 40 -- the halving stops at 2 x 35 pixels).  That is why 128 x 576 is here.  128 x 574 (window 5 as well) has cols % 4 = 2 and
  cols % 64 = 62: k_threshold_pyr's last tile column takes its right-edge branch, which loads row + cols - 4 from the caller's rows.
      switches                              240x320 232x312 222x318 227x321        128x576, 128x574
      default, B = 2                        k_threshold_mfma                       k_threshold_pyr<5> (+ the leading exact /2 levels: 4, 1)
      default, B = 8; threshold_mfma 1      k_threshold_mfma                       k_threshold_mfma
      threshold_mfma 0                      k_adaptive_threshold<7> (the box)      k_threshold_pyr<5>
      threshold_mfma 0, threshold_pyr 0     k_adaptive_threshold<7>                k_adaptive_threshold<7>
  Detector pyramid, level 1 from the caller's rows (where k_threshold_pyr does not write it), by layout:
      size      levels (exact?)                   tight          control        odd            mod4           mod8           step8
      240x320   160x120 e, 80x60 e, 40x30 e       k_half_pyr<3>  k_half_pyr<3>  k_half_area    k_half_area    k_half_pyr<3>  k_half_pyr<3>
      232x312   156x116 e, 78x58 e, 39x29 e       k_half_pyr<3>  k_half_pyr<3>  k_half_area    k_half_area    k_half_pyr<3>  k_half_pyr<3>
      222x318   159x111 e, 79x55 i, 39x27 i       k_half_area    k_half_area4   k_half_area    k_half_area    k_half_area    k_half_area4 (*)
      227x321   160x113 i, 80x56 i, 40x28 e       k_resize_level on every layout
      128x576   288x64 .. 36x8, all e             k_half_pyr<4>  k_half_pyr<4>  k_half_area    k_half_area    k_half_pyr<3>  k_half_pyr<3>
      128x574   287x64 e, 143x32 i, 71 i, 35 i    k_half_area    k_half_area4   k_half_area    k_half_area    k_half_area    k_half_area4
    with half_pyr 0 every k_half_pyr entry becomes k_half_area4.  (*) reads 8 * ceil(159 / 4) = 320 bytes of a 318-pixel row: slack.
    Levels >= 2 come from the detector's own pyramid block (k_half_area4 where exact, else k_resize_level) and see no caller layout.
    The choice is plan_pyramid_kernels (detector_plan.hpp); tests/test_input_layout_cpu.py asserts this table against it level by
    level, without a GPU -- on gfx950 a misaligned 8- or 16-byte load returns the same bytes, so no output can tell the branches apart.
  Reduced working image (DM_NORMAL, minMarkerSize 0.06, CORNER_SUBPIX): 0.06 x 320 = 19 pixels is below the 20 at which work_size()
  starts to reduce, so the case runs at 128 x 576 (-> 76 x 340): k_resize_nearest, the pyramid from the full frame and the sub-pixel
  passes read the caller's rows on layout odd.
  k_fixed_threshold's byte branch for misaligned rows cannot be reached from a device pointer: only DM_FAST / DM_VIDEO_FAST handles
  use a fixed threshold, and orbfe_aruco_detect_batch_device refuses those (frame-sequential).  It is left alone.
  orbfe_pipeline_step takes a base and a pitch (frames rows * pitch apart) and forwards them to the two engines: one step each on the
  pitches of layouts odd and step8 against the tight one.
DESIGN.md ("Device-pointer layouts") records the kernel names a rocprofv3 --kernel-trace run of this file showed."""
import numpy as np
import pytest

import device_layouts as dl
from orb_slam2_aruco_amd import synth
from pose_opt_device import Dev

pytestmark = pytest.mark.gpu

SIZES = [(240, 320), (232, 312), (222, 318), (227, 321)]
DET_SIZES = SIZES + [(128, 576), (128, 574)]
BATCHES = [2, 8]
LAYOUT_NAMES = [n for n, _, _, _ in dl.layouts(320)]
SENTINEL = 0xA5
# detector switch sets (orbfe_aruco_debug_control), reset to DEFAULTS after every case
DEFAULTS = {"threshold_mfma": -1, "threshold_pyr": 1, "half_pyr": 1}
SWITCHES = [
    ("default", {}),
    ("mfma", {"threshold_mfma": 1}),
    ("no_mfma", {"threshold_mfma": 0}),
    ("box", {"threshold_mfma": 0, "threshold_pyr": 0}),
    ("area_chain", {"threshold_mfma": 1, "half_pyr": 0}),
]

_cache = {}


def _frames(rows, cols):
    """8 scenes of the size (the first 2 are the B = 2 batch), computed once and never written."""
    key = ("frames", rows, cols)
    if key not in _cache:
        f = np.stack([synth.scene(rows, cols, 100 + i, n_markers=2, side_range=(40, min(70, rows // 2)))[0] for i in range(8)])
        f.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def _layout(cols, name):
    return next((b, s, g) for n, b, s, g in dl.layouts(cols) if n == name)


def _fills(name):
    return [0x00 if LAYOUT_NAMES.index(name) % 2 == 0 else 0xFF, dl.RANDOM]


# ---------------------------------------------------------------------------------------------------------------- extractor

def _extractor(orbfe):
    if "ex" not in _cache:
        _cache["ex"] = orbfe.ORBextractor(300, 1.2, 4, 20, 7)
    return _cache["ex"]


def _stages(ex, B):
    """every stage read-back of the last batch, as bytes: per frame and level the image, the blurred image, the FAST candidates, the
    quadtree's keypoints"""
    out = []
    for f in range(B):
        for l in range(ex.nlevels):
            out.append((ex.level_image(f, l).tobytes(), ex.level_image(f, l, True).tobytes(), ex.level_keypoints(f, l, 0).tobytes(),
                        ex.level_keypoints(f, l, 1).tobytes()))
    return out


def _extract_reference(orbfe, rows, cols, B):
    key = ("ex_ref", rows, cols, B)
    if key not in _cache:
        ex = _extractor(orbfe)
        res = ex.extract_batch(_frames(rows, cols)[:B])
        _cache[key] = (res, _stages(ex, B))
    return _cache[key]


@pytest.mark.parametrize("name", LAYOUT_NAMES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("rows,cols", SIZES)
def test_extractor_on_device_layouts(orbfe, oracle, rows, cols, B, name):
    frames = _frames(rows, cols)[:B]
    want, want_stages = _extract_reference(orbfe, rows, cols, B)
    assert max(len(k) for k, _ in want) > 50
    ex = _extractor(orbfe)
    cap = ex.capacity
    base, step, gap = _layout(cols, name)
    results = []
    for fill in _fills(name):
        host = dl.pack(frames, base, step, gap, fill, seed=rows + B)
        d_img = Dev(host)
        d_kps, d_desc = Dev(np.full(B * cap * orbfe.KP_DTYPE.itemsize, SENTINEL, np.uint8)), Dev(np.full(B * cap * 32, SENTINEL, np.uint8))
        d_n = Dev(np.full(B, -7, np.int32))
        ex.extract_batch_device(d_img.ptr + base, B, dl.frame_stride(rows, step, gap), rows, cols, step, d_kps.ptr, d_desc.ptr, cap, d_n.ptr, None)
        n = d_n.get()                                                     # (blocking: waits for the null stream)
        assert ex.batch_status() == 0
        kps, desc = d_kps.get().reshape(B, cap, -1), d_desc.get().reshape(B, cap, 32)
        assert np.array_equal(n, [len(k) for k, _ in want]), (fill, n)
        for f in range(B):
            wk, wd = want[f]
            assert kps[f, :n[f]].tobytes() == wk.tobytes(), (fill, f)     # every field of every keypoint, bit for bit
            assert np.array_equal(desc[f, :n[f]], wd), (fill, f)
            assert (kps[f, n[f]:] == SENTINEL).all() and (desc[f, n[f]:] == SENTINEL).all(), (fill, f)   # records past n: untouched
        got_stages = _stages(ex, B)
        for i, (g, w) in enumerate(zip(got_stages, want_stages)):
            for what, a, b in zip(("image", "blurred image", "FAST candidates", "quadtree keypoints"), g, w):
                assert a == b, "%s of frame %d level %d differs (fill %r)" % (what, i // ex.nlevels, i % ex.nlevels, fill)
        assert np.array_equal(d_img.get(), host), "the call wrote the caller's buffer (fill %r)" % (fill,)
        results.append((n.tobytes(), kps.tobytes(), desc.tobytes(), got_stages))
    assert results[0] == results[1], "the slack's content changed the output"
    if (rows, cols) == (240, 320):                                         # the reference's own arithmetic (the CPU oracle)
        ora = oracle.OrbOracle(300, 1.2, 4, 20, 7)
        for f in range(B):
            okps, odesc = ora.extract(frames[f])
            gk = np.frombuffer(results[0][1], orbfe.KP_DTYPE).reshape(B, cap)[f, :len(okps)]
            assert len(okps) == len(want[f][0])
            for fld in ("x", "y", "size", "response", "octave"):
                assert np.array_equal(gk[fld], okps[fld]), (f, fld)
            assert np.allclose(gk["angle"], okps["angle"], atol=1e-4)
            assert np.array_equal(np.frombuffer(results[0][2], np.uint8).reshape(B, cap, 32)[f, :len(okps)], odesc), f


# ----------------------------------------------------------------------------------------------------------------- detector

def _detector(orbfe, key="det"):
    if key not in _cache:
        _cache[key] = orbfe.MarkerDetector("ARUCO")
    return _cache[key]


def _mean_pyramid(img):
    """numpy's rounded 2 x 2 mean while a level halves exactly (buildPyramid's exact levels; the halving stops at 2 x 35 pixels)"""
    out, ref, tw = [], img, img.shape[1]
    while tw > 70:
        tw //= 2
        if ref.shape[0] % 2 or ref.shape[1] % 2:
            break
        a = ref.astype(np.uint16)
        ref = ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        out.append(ref)
    return out


def _levels(det, rows, cols, f):
    """the detector's pyramid levels >= 1 of frame f of the last batch (all of them: inexact ones included), as arrays.
    pyramid_level() cuts the read-back to (h // 2, w // 2) per level, which is the plan's size of a level, exact or not (lw /= 2,
    lh /= 2 in plan_detector): the arrays are whole levels, compared here between host-pointer and device-pointer calls only."""
    out, w, h, tw, level = [], cols, rows, cols, 1
    while tw > 70:
        tw //= 2; w //= 2; h //= 2
        if w < 1 or h < 1:
            break
        out.append(det.pyramid_level(level, f))
        assert out[-1] is not None and out[-1].shape == (h, w), (level, out[-1] is None)
        level += 1
    assert det.pyramid_level(level, f) is None
    return out


def _detect_reference(orbfe, rows, cols, B):
    """host-pointer detect_batch with the default switches: markers, threshold images, pyramid levels of every frame"""
    key = ("det_ref", rows, cols, B)
    if key not in _cache:
        det = _detector(orbfe)
        frames = _frames(rows, cols)[:B]
        mk = det.detect_batch(frames)
        thr = [det.thresholded(f).tobytes() for f in range(B)]
        lv = [_levels(det, rows, cols, f) for f in range(B)]
        for f in range(B):                                                 # the exact levels are numpy's 2 x 2 mean
            mean = _mean_pyramid(frames[f])
            assert len(mean) >= 1 or cols % 2 or rows % 2
            for l, m in enumerate(mean):
                assert np.array_equal(lv[f][l], m), (f, l)
        _cache[key] = (mk, thr, [[a.tobytes() for a in fl] for fl in lv])
    return _cache[key]


def _run_detector(orbfe, det, d_img, base, B, rows, cols, step, gap):
    cap = det.capacity
    d_out = Dev(np.full(B * cap * orbfe.MARKER_DTYPE.itemsize, SENTINEL, np.uint8))
    d_n = Dev(np.full(B, -7, np.int32))
    det.detect_batch_device(d_img.ptr + base, B, dl.frame_stride(rows, step, gap), rows, cols, step, d_out.ptr, cap, d_n.ptr, None)
    n = d_n.get()
    assert det.batch_status() == (0, 0)
    return n, d_out.get().reshape(B, cap, -1)


def _check_markers(n, rec, want, what):
    assert np.array_equal(n, [len(m) for m in want]), (what, n)
    for f, m in enumerate(want):
        assert rec[f, :n[f]].tobytes() == m.tobytes(), (what, f)           # ids and corners, bit for bit
        assert (rec[f, n[f]:] == SENTINEL).all(), (what, f)                # records past n: untouched


@pytest.mark.parametrize("name", LAYOUT_NAMES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("rows,cols", DET_SIZES)
def test_detector_on_device_layouts(orbfe, rows, cols, B, name):
    frames = _frames(rows, cols)[:B]
    want, want_thr, want_lv = _detect_reference(orbfe, rows, cols, B)
    assert max(len(m) for m in want) >= 1
    det = _detector(orbfe)
    base, step, gap = _layout(cols, name)
    try:
        per_fill = []
        for fill in _fills(name):
            host = dl.pack(frames, base, step, gap, fill, seed=cols + B)
            d_img = Dev(host)
            outs = []
            for sw_name, sw in SWITCHES:
                for k, v in {**DEFAULTS, **sw}.items():
                    det.debug_control(k, v)
                what = (sw_name, fill)
                n, rec = _run_detector(orbfe, det, d_img, base, B, rows, cols, step, gap)
                _check_markers(n, rec, want, what)
                thr = [det.thresholded(f).tobytes() for f in range(B)]
                lv = [[a.tobytes() for a in _levels(det, rows, cols, f)] for f in range(B)]
                assert thr == want_thr, what                               # the adaptive threshold is integer arithmetic in every kernel
                assert lv == want_lv, what                                 # and so is every pyramid kernel
                assert np.array_equal(d_img.get(), host), "the call wrote the caller's buffer %r" % (what,)
                outs.append((n.tobytes(), rec.tobytes(), thr, lv))
            per_fill.append(outs)
        assert per_fill[0] == per_fill[1], "the slack's content changed the output"
    finally:
        for k, v in DEFAULTS.items():
            det.debug_control(k, v)


def test_batches_hold_markers_and_keypoints(orbfe):
    """what the cases above stand on: every batch has a frame with a marker, and (the extractor's sizes) with more than 50 keypoints"""
    for rows, cols in DET_SIZES:
        for B in BATCHES:
            assert max(len(m) for m in _detect_reference(orbfe, rows, cols, B)[0]) >= 1, (rows, cols, B)
            if (rows, cols) in SIZES:
                assert max(len(k) for k, _ in _extract_reference(orbfe, rows, cols, B)[0]) > 50, (rows, cols, B)


@pytest.mark.parametrize("B", BATCHES)
def test_reduced_working_image_on_an_odd_layout(orbfe, B):
    """The stateless reduced mode: k_resize_nearest, the pyramid, the patch warps and the sub-pixel passes read the caller's frame."""
    rows, cols = 128, 576
    frames = _frames(rows, cols)[:B]
    det = _detector(orbfe, "det_reduced")
    det.setCornerRefinementMethod(det.CORNER_SUBPIX)
    det.setDetectionMode(det.DM_NORMAL, 0.06)
    want = det.detect_batch(frames)
    assert det.state()["work_shape"] == (76, 340)                          # the mode does reduce at this size
    assert max(len(m) for m in want) >= 1
    base, step, gap = _layout(cols, "odd")
    outs = []
    for fill in _fills("odd"):
        host = dl.pack(frames, base, step, gap, fill, seed=B)
        d_img = Dev(host)
        n, rec = _run_detector(orbfe, det, d_img, base, B, rows, cols, step, gap)
        _check_markers(n, rec, want, fill)
        assert np.array_equal(d_img.get(), host), "the call wrote the caller's buffer (fill %r)" % (fill,)
        outs.append((n.tobytes(), rec.tobytes()))
    assert outs[0] == outs[1], "the slack's content changed the output"


# ----------------------------------------------------------------------------------------------------------------- pipeline

def test_pipeline_step_on_unaligned_pitches(orbfe):
    """orbfe_pipeline_step forwards base and pitch to both engines: a step on frames at base 1 with pitch cols + 1, and one at the next
    multiple of 8 above cols, give the records of the step on tightly packed frames -- keypoints, descriptors, markers, poses of every
    frame, and the matches between the batch's frames -- and leave the buffer as it was.  A pitch below cols is refused by the layout
    check, in front of everything else."""
    from orb_slam2_aruco_amd import pipeline
    rows, cols, B = 240, 320, 2
    frames = _frames(rows, cols)[:B]
    pipe = pipeline.FrontEndPipeline(B, rows, cols, nfeatures=300, nlevels=4)
    got = []
    for name in ("tight", "odd", "step8"):
        base, step, _ = _layout(cols, name)
        for fill in _fills(name) if name != "tight" else [0x00]:
            host = dl.pack(frames, base, step, 0, fill, seed=5)
            d_img = Dev(host)
            pipe.reset_stream()                                            # every step is the first of its stream: no frame in front
            cur = pipe.step_ptr(d_img.ptr + base, step)
            rec = pipeline.valid_records(pipe.read_records(cur))
            m = pipe.read_matches()
            assert not any(pipe.status().values())
            assert np.array_equal(d_img.get(), host), (name, fill)
            pairs = [(int(m["nmatches"][p]), m["matches12"][p, :rec[p - 1][0]].tobytes()) for p in range(1, B)]
            got.append((name, fill, rec, pairs))
    assert max(r[0] for r in got[0][2]) > 50 and max(r[3] for r in got[0][2]) >= 1     # keypoints and a marker in the batch
    for name, fill, rec, pairs in got[1:]:
        assert rec == got[0][2], (name, fill)
        assert pairs == got[0][3], (name, fill)
    d_img = Dev(dl.pack(frames, 0, cols, 0, 0x00))
    with pytest.raises(orbfe.OrbfeError, match="input layout: row step"):
        pipe.step_ptr(d_img.ptr, cols - 1)
