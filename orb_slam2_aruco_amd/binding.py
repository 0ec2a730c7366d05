"""ctypes binding of liborbfe.so (the C ABI of include/orbfe.h).

This is plumbing for tests and bench.py; the product is the shared library.  There is no Python or CPU
implementation behind these classes: if the library is missing or no HIP device is usable, construction fails.
"""
import ctypes as C
import os

import numpy as np

from . import header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBFE_LIB", os.path.join(_HERE, "liborbfe.so"))

KP_DTYPE = header.dtype("orbfe_keypoint")
MARKER_DTYPE = header.dtype("orbfe_marker")
POSE_DTYPE = header.dtype("orbfe_marker_pose")
assert KP_DTYPE.itemsize == 28 and MARKER_DTYPE.itemsize == 36

# every function include/orbfe.h declares (tests/test_abi_cpu.py checks them against what the .so exports)
SYMBOLS = list(header.functions)

_lib = None


def _defines(*names):
    return [header.defines[n] for n in names]


# return codes of include/orbfe.h
ORBFE_OK, ORBFE_ERR_INVALID, ORBFE_ERR_NO_DEVICE, ORBFE_ERR_HIP, ORBFE_ERR_CAPACITY, ORBFE_ERR_DICT = _defines(
    "OK", "ERR_INVALID", "ERR_NO_DEVICE", "ERR_HIP", "ERR_CAPACITY", "ERR_DICT")
# ORBFE_ARUCO_FLAG_TRUNCATED: a frame of a device batch had more markers than the caller's capacity (MarkerDetector.batch_status,
# FrontEndPipeline.status); every other flag bit is an internal capacity of the detector
ARUCO_FLAG_TRUNCATED = header.defines["ARUCO_FLAG_TRUNCATED"]


class OrbfeError(RuntimeError):
    pass


def load():
    """Load liborbfe.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OrbfeError("%s not found: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950)"
                         % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in header.functions.items():     # a partial library (a test build of some engines) is accepted
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(L, rc, what):
    if rc < 0:
        raise OrbfeError("%s failed (%d): %s" % (what, rc, L.orbfe_last_error().decode()))
    return rc


class ORBextractor:
    """Mirror of ORB_SLAM2::ORBextractor (reference include/ORBextractor.h:45-113) over the C ABI."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, device=0):
        self.L = load()
        self.nlevels = nlevels
        self.h = self.L.orbfe_extractor_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device)
        if not self.h:
            raise OrbfeError("orbfe_extractor_create: " + self.L.orbfe_last_error().decode())
        self.capacity = self.L.orbfe_extractor_max_keypoints(self.h)

    @classmethod
    def wrap(cls, handle, nlevels):
        """A non-owning view of an extractor another object owns (the engines of an orbfe_pipeline)."""
        self = cls.__new__(cls)
        self.L = load()
        self.nlevels = nlevels
        self.h = handle
        self._borrowed = True
        self.capacity = self.L.orbfe_extractor_max_keypoints(self.h)
        return self

    def __del__(self):
        if getattr(self, "h", None) and not getattr(self, "_borrowed", False):
            self.L.orbfe_extractor_destroy(self.h)
        self.h = None

    # reference getters (ORBextractor.h:63-83)
    def GetLevels(self):
        return self.L.orbfe_extractor_get_levels(self.h)

    def GetScaleFactor(self):
        return self.L.orbfe_extractor_get_scale_factor(self.h)

    def _vec(self, name, dtype=np.float32):
        out = np.zeros(self.nlevels, dtype)
        _check(self.L, getattr(self.L, "orbfe_extractor_get_" + name)(self.h, _p(out)), name)
        return out

    def GetScaleFactors(self):
        return self._vec("scale_factors")

    def GetInverseScaleFactors(self):
        return self._vec("inverse_scale_factors")

    def GetScaleSigmaSquares(self):
        return self._vec("scale_sigma_squares")

    def GetInverseScaleSigmaSquares(self):
        return self._vec("inverse_scale_sigma_squares")

    def features_per_level(self):
        return self._vec("features_per_level", np.int32)

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors): returns (keypoints[KP_DTYPE], descriptors[n,32])."""
        image = np.asarray(image)
        if image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2, "CV_8UC1 expected (ORBextractor.cc:1050)"
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        kps = np.zeros(self.capacity, KP_DTYPE)
        desc = np.zeros((self.capacity, 32), np.uint8)
        n = C.c_int32(0)
        _check(self.L, self.L.orbfe_extract(self.h, _p(image), image.shape[0], image.shape[1], image.strides[0],
                                            _p(kps), _p(desc), self.capacity, C.byref(n)), "orbfe_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch(self, images):
        """images: (B, rows, cols) uint8 host array. Returns list of (kps, desc)."""
        images = np.ascontiguousarray(images, np.uint8)
        B, rows, cols = images.shape
        kps = np.zeros((B, self.capacity), KP_DTYPE)
        desc = np.zeros((B, self.capacity, 32), np.uint8)
        n = np.zeros(B, np.int32)
        _check(self.L, self.L.orbfe_extract_batch(self.h, _p(images), B, images.strides[0], rows, cols,
                                                  images.strides[1], _p(kps), _p(desc), self.capacity, _p(n)),
               "orbfe_extract_batch")
        return [(kps[f, :n[f]].copy(), desc[f, :n[f]].copy()) for f in range(B)]

    def extract_batch_device(self, d_imgs_ptr, B, frame_stride, rows, cols, step, d_kps_ptr, d_desc_ptr, capacity,
                             d_n_ptr, stream=0):
        _check(self.L, self.L.orbfe_extract_batch_device(self.h, d_imgs_ptr, B, frame_stride, rows, cols, step,
                                                         d_kps_ptr, d_desc_ptr, capacity, d_n_ptr, stream),
               "orbfe_extract_batch_device")

    def set_gaussian_taps(self, mode):
        """0: taps 18 34 49 55 49 34 18 (OpenCV 2.4 / 3.2 / early 3.4); 1: 18 34 48 56 48 34 18 (late 3.4.x / 4.x)."""
        _check(self.L, self.L.orbfe_extractor_set_gaussian_taps(self.h, int(mode)), "orbfe_extractor_set_gaussian_taps")

    def batch_status(self):
        """0, or the largest per-frame keypoint total of the last device batch that did not fit its capacity."""
        ovf = C.c_int32(0)
        _check(self.L, self.L.orbfe_extractor_batch_status(self.h, C.byref(ovf)), "orbfe_extractor_batch_status")
        return ovf.value

    # stage read-back for parity tests
    def level_image(self, frame, level, blurred=False):
        w, h = C.c_int(), C.c_int()
        _check(self.L, self.L.orbfe_extractor_debug_level_size(self.h, level, C.byref(w), C.byref(h)), "level_size")
        out = np.zeros((h.value, w.value), np.uint8)
        _check(self.L, self.L.orbfe_extractor_debug_level_image(self.h, frame, level, int(blurred), _p(out)),
               "level_image")
        return out

    def level_keypoints(self, frame, level, stage):
        n = C.c_int32(0)
        _check(self.L, self.L.orbfe_extractor_debug_level_keypoints(self.h, frame, level, stage, None, 0, C.byref(n)),
               "level_keypoints")
        out = np.zeros(max(n.value, 1), KP_DTYPE)
        _check(self.L, self.L.orbfe_extractor_debug_level_keypoints(self.h, frame, level, stage, _p(out), n.value,
                                                                    C.byref(n)), "level_keypoints")
        return out[:n.value]

    def level_sizes(self):
        out = []
        for l in range(self.nlevels):
            w, h = C.c_int(), C.c_int()
            _check(self.L, self.L.orbfe_extractor_debug_level_size(self.h, l, C.byref(w), C.byref(h)), "level_size")
            out.append((w.value, h.value))
        return out

    def set_aux_stream(self, stream_ptr):
        """Run the extractor's forked launch (blur) on the caller's stream (None: the handle's own)."""
        _check(self.L, self.L.orbfe_extractor_set_aux_stream(self.h, stream_ptr), "set_aux_stream")

    def pair_detector(self, detector):
        """Start `detector` (a MarkerDetector or None) on every single frame this extractor is given: the detector's next detect()
        of the same image finds its work done (orbfe_extractor_pair_detector)."""
        _check(self.L, self.L.orbfe_extractor_pair_detector(self.h, detector.h if detector is not None else None), "pair_detector")
        self._paired = detector      # keeps the detector alive as long as it is paired

    def follow(self, other, stage):
        """Every batch of this handle starts behind stage 1 (FAST) / 2 (quadtree) / 3 (descriptors) of `other`'s latest batch; 0: free."""
        _check(self.L, self.L.orbfe_extractor_follow(self.h, other.h if other is not None else None, int(stage)), "follow")
        self._followed = other

    def debug_control(self, key, value):
        """orbfe_extractor_debug_control: a named test / diagnosis switch of this handle (include/orbfe.h lists the keys)."""
        _check(self.L, self.L.orbfe_extractor_debug_control(self.h, key.encode(), int(value)), "extractor_debug_control")

    def enable_kernel_timing(self, on=True):
        self.debug_control("kernel_timing", on)

    def force_general_quadtree(self, on=True):
        """Test hook: bypass the count-pyramid fast path of DistributeOctTree."""
        self.debug_control("general_quadtree", on)

    def set_pyramid_depth(self, depth=0):
        """Test hook: depth of the quadtree count pyramid (0 = default); shallow values force the fallback."""
        self.debug_control("pyramid_depth", depth)

    def quadtree_fell_back(self, frame, level):
        n = C.c_int32(0)
        _check(self.L, self.L.orbfe_extractor_debug_level_keypoints(self.h, frame, level, 3, None, 0, C.byref(n)),
               "level_keypoints")
        return bool(n.value)

    # order of kernel_times_us(); blur7 runs on the extractor's second stream, concurrently with fast_cells + distribute
    STAGES = ["resize", "blur7", "fast_cells", "distribute", "orient_describe"]

    @classmethod
    def stage_names(cls, n):
        """The names of n stage times (every batch times the same stages: STAGES)."""
        return cls.STAGES

    def kernel_times_us(self, median=False):
        """Stage times of the last batch, or (median=True) the per-stage median over the batches since timing was enabled."""
        out = np.zeros(32, np.float32)
        n = self.L.orbfe_extractor_debug_kernel_times(self.h, _p(out), -32 if median else 32)
        return out[:n]


# ------------------------------------------------------------------------------------------ matching --
def hamming(a, b):
    L = load()
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
    return L.orbfe_hamming(_p(a), _p(b))


def knn2_csr(Q, T, offsets, idx, init=256, device=0):
    """Best / second-best of every query over its own candidate list (CSR)."""
    L = load()
    Q = np.ascontiguousarray(Q, np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, np.uint8).reshape(-1, 32)
    offsets = np.ascontiguousarray(offsets, np.int32); idx = np.ascontiguousarray(idx, np.int32)
    bi = np.full(len(Q), -1, np.int32); bd = np.full(len(Q), init, np.int32); sd = np.full(len(Q), init, np.int32)
    _check(L, L.orbfe_knn2_csr(_p(Q), len(Q), _p(T), len(T), _p(offsets), _p(idx), init, _p(bi), _p(bd), _p(sd), device),
           "orbfe_knn2_csr")
    return bi, bd, sd


def debug_control(key, value):
    L = load()
    _check(L, L.orbfe_debug_control(key.encode(), int(value)), "orbfe_debug_control")


def distinctive_descriptors(desc, offsets, device=0):
    """MapPoint::ComputeDistinctiveDescriptors over many map points (MapPoint.cc:270-333) -> (best index per point, chosen descriptors)."""
    L = load()
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    o = np.ascontiguousarray(offsets, np.int32)
    n = len(o) - 1
    bi = np.full(max(n, 1), -1, np.int32); bd = np.zeros((max(n, 1), 32), np.uint8)
    _check(L, L.orbfe_distinctive_descriptors(_p(d) if len(d) else None, _p(o), n, _p(bi), _p(bd), device), "orbfe_distinctive_descriptors")
    return bi[:n], bd[:n]


def knn2(Q, T, init=256, device=0):
    """All-pairs best / second-best (ORBmatcher inner loop). Returns (best_idx, best_dist, second_dist)."""
    L = load()
    Q = np.ascontiguousarray(Q, np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, np.uint8).reshape(-1, 32)
    bi = np.full(len(Q), -1, np.int32); bd = np.full(len(Q), init, np.int32); sd = np.full(len(Q), init, np.int32)
    _check(L, L.orbfe_knn2(_p(Q), len(Q), _p(T), len(T), init, _p(bi), _p(bd), _p(sd), device), "orbfe_knn2")
    return bi, bd, sd


WINDOW_QUERY_DTYPE = header.dtype("orbfe_window_query")


def search_by_projection(kps, desc, cols, rows, queries, qdesc, taken=None, mode=0, th_high=100, nnratio=0.8, device=0,
                         bounds=None, q_observed=None):
    """The matching loop of ORBmatcher::SearchByProjection(Frame&, vpMapPoints, th) (ORBmatcher.cc:45-129) on flat arrays:
    queries = WINDOW_QUERY_DTYPE records (projected position, radius, octave range), qdesc = their descriptors.
    mode 0: best / second-best + octaves per query; mode 1: the whole loop (accept rule, taken keypoints)."""
    L = load()
    kps = np.ascontiguousarray(kps, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    queries = np.ascontiguousarray(queries, WINDOW_QUERY_DTYPE); qdesc = np.ascontiguousarray(qdesc, np.uint8)
    nq = len(queries)
    tk = None if taken is None else np.ascontiguousarray(taken, np.uint8).copy()
    out = [np.zeros(max(nq, 1), np.int32) for _ in range(6)]
    nm = C.c_int32(0)
    bnd = None if bounds is None else np.ascontiguousarray(bounds, np.float32)
    _check(L, L.orbfe_search_by_projection(_p(kps), _p(desc), len(kps), cols, rows, None if bnd is None else _p(bnd),
                                           _p(queries), _p(qdesc), nq,
                                           None if tk is None else _p(tk),
                                           None if q_observed is None else _p(np.ascontiguousarray(q_observed, np.uint8)),
                                           mode, th_high, nnratio, *[_p(o) for o in out],
                                           C.byref(nm), device), "orbfe_search_by_projection")
    return dict(best_idx=out[0][:nq], best_dist=out[1][:nq], best_level=out[2][:nq], second_dist=out[3][:nq],
                second_level=out[4][:nq], match=out[5][:nq], nmatches=nm.value, taken=tk)


def _camera(K, dist):
    """K: 3x3 matrix or (fx, fy, cx, cy); dist: mDistCoef (4 or 5 values, up to 12)."""
    K = np.asarray(K, np.float32)
    K4 = np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.ndim == 2 else K.reshape(4), np.float32)
    d = np.ascontiguousarray(np.asarray([] if dist is None else dist, np.float32).reshape(-1))
    return K4, d


def undistort_points(pts, K, dist, device=0):
    """cv::undistortPoints(pts, K, dist, R=I, P=K) on an (n, 2) float array (Frame.cc:357-416)."""
    L = load()
    K4, d = _camera(K, dist)
    src = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    dst = np.empty_like(src)
    _check(L, L.orbfe_undistort_points(_p(src), len(src), _p(K4), _p(d) if len(d) else None, len(d), _p(dst), device),
           "orbfe_undistort_points")
    return dst


def UndistortKeyPoints(kps, K, dist, device=0):
    """Frame::UndistortKeyPoints (Frame.cc:357-387): mvKeysUn = mvKeys with (x, y) undistorted; unchanged when dist[0] == 0."""
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    K4, d = _camera(K, dist)
    if len(d) == 0 or d[0] == 0.0 or len(kps) == 0:
        return kps.copy()
    un = kps.copy()
    xy = undistort_points(np.stack([kps["x"], kps["y"]], 1), K4, d, device)
    un["x"] = xy[:, 0]; un["y"] = xy[:, 1]
    return un


def ComputeImageBounds(cols, rows, K, dist, device=0):
    """Frame::ComputeImageBounds (Frame.cc:418-451) -> float32 [mnMinX, mnMinY, mnMaxX, mnMaxY] (the `bounds` of the searches)."""
    L = load()
    K4, d = _camera(K, dist)
    out = np.zeros(4, np.float32)
    _check(L, L.orbfe_compute_image_bounds(cols, rows, _p(K4), _p(d) if len(d) else None, len(d), _p(out), device),
           "orbfe_compute_image_bounds")
    return out


def search_by_projection_last_frame(kps_cur, desc_cur, cols, rows, kps_last, valid_last, x3Dw, mp_desc, Tcw, K4, scale_factors, th,
                                    taken_cur=None, mp_observed=None, th_high=100, check_orientation=True, bounds=None, device=0):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, mono) (ORBmatcher.cc:1332-1474) -> (nmatches, match_cur)."""
    L = load()
    kc = np.ascontiguousarray(kps_cur, KP_DTYPE); dc = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
    kl = np.ascontiguousarray(kps_last, KP_DTYPE)
    opt = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    vl, tc, ob, bnd = opt(valid_last, np.uint8), opt(taken_cur, np.uint8), opt(mp_observed, np.uint8), opt(bounds, np.float32)
    x = np.ascontiguousarray(x3Dw, np.float32).reshape(-1, 3); md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(-1)[:12].copy(); K = np.ascontiguousarray(K4, np.float32)
    sf = np.ascontiguousarray(scale_factors, np.float32)
    m = np.full(len(kc), -1, np.int32); nm = C.c_int32(0)
    pp = lambda a: None if a is None else _p(a)
    _check(L, L.orbfe_search_by_projection_last_frame(_p(kc), _p(dc), len(kc), pp(tc), cols, rows, pp(bnd), _p(kl), len(kl), pp(vl), _p(x),
                                                      _p(md), pp(ob), _p(T), _p(K), _p(sf), len(sf), th, th_high, int(check_orientation),
                                                      _p(m), C.byref(nm), device), "orbfe_search_by_projection_last_frame")
    return nm.value, m


def search_by_projection_best(kps, desc, cols, rows, queries, q_angle, qdesc, th_high, factor, q_blocks=None, taken=None,
                              check_orientation=True, bounds=None, device=0):
    """Best-only guided search with rotation consistency (ORBmatcher.cc:1476-1603 and relatives) -> (nmatches, match_cur)."""
    L = load()
    k = np.ascontiguousarray(kps, KP_DTYPE); d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    q = np.ascontiguousarray(queries, WINDOW_QUERY_DTYPE); qa = np.ascontiguousarray(q_angle, np.float32)
    qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    opt = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    qb, tk, bnd = opt(q_blocks, np.uint8), opt(taken, np.uint8), opt(bounds, np.float32)
    pp = lambda a: None if a is None else _p(a)
    m = np.full(len(k), -1, np.int32); nm = C.c_int32(0)
    _check(L, L.orbfe_search_by_projection_best(_p(k), _p(d), len(k), cols, rows, pp(bnd), _p(q), _p(qa), _p(qd), pp(qb), len(q), pp(tk),
                                                th_high, int(check_orientation), np.float32(factor), _p(m), C.byref(nm), device),
           "orbfe_search_by_projection_best")
    return nm.value, m


def fuse_search(kps, desc, cols, rows, p3Dw, valid, min_dist, max_dist, normal, mp_desc, Tcw, Ow, K4, scale_factors, inv_level_sigma2,
                log_scale_factor, th, chi2=5.99, bounds=None, device=0):
    """Matching part of ORBmatcher::Fuse (ORBmatcher.cc:829-970; chi2=0: the Scw variant :972-1104) -> (best_idx, best_dist)."""
    L = load()
    k = np.ascontiguousarray(kps, KP_DTYPE); d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    f = lambda a, t=np.float32: np.ascontiguousarray(a, t)
    x, mn, mx, nr, md = f(p3Dw).reshape(-1, 3), f(min_dist), f(max_dist), f(normal).reshape(-1, 3), f(mp_desc, np.uint8).reshape(-1, 32)
    v = None if valid is None else f(valid, np.uint8); bnd = None if bounds is None else f(bounds)
    T, O, K, sf, isg = f(Tcw).reshape(-1)[:12].copy(), f(Ow), f(K4), f(scale_factors), f(inv_level_sigma2)
    bi = np.full(len(x), -1, np.int32); bd = np.full(len(x), 256, np.int32)
    pp = lambda a: None if a is None else _p(a)
    _check(L, L.orbfe_fuse_search(_p(k), _p(d), len(k), cols, rows, pp(bnd), _p(x), pp(v), _p(mn), _p(mx), _p(nr), _p(md), len(x), _p(T), _p(O),
                                  _p(K), _p(sf), _p(isg), len(sf), log_scale_factor, th, float(chi2), _p(bi), _p(bd), device), "orbfe_fuse_search")
    return bi, bd


def search_by_projection_keyframe(kps_cur, desc_cur, cols, rows, kf_angle, valid, p3Dw, min_dist, max_dist, mp_desc, Tcw, Ow, K4, scale_factors,
                                  log_scale_factor, th, orb_dist, taken_cur=None, check_orientation=True, bounds=None, device=0):
    """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1476-1603) -> (nmatches, match_cur)."""
    L = load()
    kc = np.ascontiguousarray(kps_cur, KP_DTYPE); dc = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
    f = lambda a, t=np.float32: np.ascontiguousarray(a, t)
    x, mn, mx, md, ang = f(p3Dw).reshape(-1, 3), f(min_dist), f(max_dist), f(mp_desc, np.uint8).reshape(-1, 32), f(kf_angle)
    opt = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    v, tc, bnd = opt(valid, np.uint8), opt(taken_cur, np.uint8), opt(bounds, np.float32)
    T, O, K, sf = f(Tcw).reshape(-1)[:12].copy(), f(Ow), f(K4), f(scale_factors)
    m = np.full(len(kc), -1, np.int32); nm = C.c_int32(0)
    pp = lambda a: None if a is None else _p(a)
    _check(L, L.orbfe_search_by_projection_keyframe(_p(kc), _p(dc), len(kc), pp(tc), cols, rows, pp(bnd), len(x), _p(ang), pp(v), _p(x), _p(mn),
                                                    _p(mx), _p(md), _p(T), _p(O), _p(K), _p(sf), len(sf), log_scale_factor, th, int(orb_dist),
                                                    int(check_orientation), _p(m), C.byref(nm), device), "orbfe_search_by_projection_keyframe")
    return nm.value, m


def project_map_points(p3Dw, valid, min_dist, max_dist, normal, Tcw, Ow, K4, cols, rows, scale_factors, log_scale_factor, th, level_below,
                       level_above, strict_max=True, bounds=None, device=0):
    """Projection + gates + PredictScale -> WINDOW_QUERY_DTYPE records (r < 0 = not searched).  strict_max=False selects the
    projection of SearchByProjection(CurrentFrame, pKF, ...) (ORBmatcher.cc:1503-1512), see orbfe.h."""
    L = load()
    f = lambda a, t=np.float32: np.ascontiguousarray(a, t)
    x, mn, mx = f(p3Dw).reshape(-1, 3), f(min_dist), f(max_dist)
    nr = None if normal is None else f(normal).reshape(-1, 3)
    v = None if valid is None else f(valid, np.uint8); bnd = None if bounds is None else f(bounds)
    T, O, K, sf = f(Tcw).reshape(-1)[:12].copy(), f(Ow), f(K4), f(scale_factors)
    q = np.zeros(len(x), WINDOW_QUERY_DTYPE)
    pp = lambda a: None if a is None else _p(a)
    _check(L, L.orbfe_project_map_points(_p(x), pp(v), _p(mn), _p(mx), pp(nr), len(x), _p(T), _p(O), _p(K), cols, rows, pp(bnd), int(strict_max),
                                         _p(sf), len(sf), log_scale_factor, th, level_below, level_above, _p(q), device), "orbfe_project_map_points")
    return q


def search_by_sim3(kf1, kf2, cols, rows, T1w, T2w, sT12, sT21, K4, scale_factors, log_scale_factor, th, th_high=100, bounds=None, device=0):
    """ORBmatcher::SearchBySim3 (ORBmatcher.cc:1106-1330).  kf = dict(kps, desc, p3Dw, valid, min_dist, max_dist, mp_desc) -> (nFound, match12)."""
    L = load()
    f = lambda a, t=np.float32: np.ascontiguousarray(a, t)
    def side(kf):
        v = None if kf.get("valid") is None else f(kf["valid"], np.uint8)
        return [np.ascontiguousarray(kf["kps"], KP_DTYPE), f(kf["desc"], np.uint8).reshape(-1, 32), f(kf["p3Dw"]).reshape(-1, 3), v,
                f(kf["min_dist"]), f(kf["max_dist"]), f(kf["mp_desc"], np.uint8).reshape(-1, 32)]
    a, b = side(kf1), side(kf2)
    pp = lambda x: None if x is None else _p(x)
    bnd = None if bounds is None else f(bounds)
    Ts = [f(T).reshape(-1)[:12].copy() for T in (T1w, T2w, sT12, sT21)]
    K, sf = f(K4), f(scale_factors)
    m12 = np.full(len(a[0]), -1, np.int32); nf = C.c_int32(0)
    _check(L, L.orbfe_search_by_sim3(_p(a[0]), _p(a[1]), len(a[0]), _p(b[0]), _p(b[1]), len(b[0]), cols, rows, pp(bnd),
                                     _p(a[2]), pp(a[3]), _p(a[4]), _p(a[5]), _p(a[6]), _p(b[2]), pp(b[3]), _p(b[4]), _p(b[5]), _p(b[6]),
                                     _p(Ts[0]), _p(Ts[1]), _p(Ts[2]), _p(Ts[3]), _p(K), _p(sf), len(sf), log_scale_factor, th, th_high,
                                     _p(m12), C.byref(nf), device), "orbfe_search_by_sim3")
    return nf.value, m12


def search_by_projection_sim3(kps, desc, cols, rows, matched, p3Dw, valid, min_dist, max_dist, normal, mp_desc, Tcw, Ow, K4, scale_factors,
                              log_scale_factor, th, bounds=None, device=0):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:294-407) -> (nmatches, match_kf)."""
    L = load()
    k = np.ascontiguousarray(kps, KP_DTYPE); d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    f = lambda a, t=np.float32: np.ascontiguousarray(a, t)
    x, mn, mx, nr, md = f(p3Dw).reshape(-1, 3), f(min_dist), f(max_dist), f(normal).reshape(-1, 3), f(mp_desc, np.uint8).reshape(-1, 32)
    v = None if valid is None else f(valid, np.uint8); bnd = None if bounds is None else f(bounds)
    mt = None if matched is None else f(matched, np.uint8)
    T, O, K, sf = f(Tcw).reshape(-1)[:12].copy(), f(Ow), f(K4), f(scale_factors)
    m = np.full(len(k), -1, np.int32); nm = C.c_int32(0)
    pp = lambda a: None if a is None else _p(a)
    _check(L, L.orbfe_search_by_projection_sim3(_p(k), _p(d), len(k), cols, rows, pp(bnd), pp(mt), _p(x), pp(v), _p(mn), _p(mx), _p(nr), _p(md),
                                                len(x), _p(T), _p(O), _p(K), _p(sf), len(sf), log_scale_factor, int(th), _p(m), C.byref(nm),
                                                device), "orbfe_search_by_projection_sim3")
    return nm.value, m


class ORBmatcher:
    """Mirror of ORB_SLAM2::ORBmatcher (reference include/ORBmatcher.h:41-83) for the rows built so far."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.mfNNratio = nnratio
        self.mbCheckOrientation = checkOri
        self.device = device
        self.L = load()

    @staticmethod
    def DescriptorDistance(a, b):
        return hamming(a, b)

    def SearchForInitialization(self, kps1, desc1, kps2, desc2, cols, rows, vbPrevMatched=None, windowSize=10, bounds=None):
        """Returns (nmatches, vnMatches12, vbPrevMatched'); frames are given as (keypoints, descriptors)."""
        k1 = np.ascontiguousarray(kps1); k2 = np.ascontiguousarray(kps2)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        if vbPrevMatched is None:
            vbPrevMatched = np.stack([k1["x"], k1["y"]], 1)
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).copy()
        m12 = np.full(len(k1), -1, np.int32)
        n = C.c_int32(0)
        bnd = None if bounds is None else np.ascontiguousarray(bounds, np.float32)
        _check(self.L, self.L.orbfe_search_for_initialization(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), cols,
                                                              rows, None if bnd is None else _p(bnd), _p(prev), _p(m12), windowSize, self.mfNNratio,
                                                              int(self.mbCheckOrientation), C.byref(n), self.device),
               "orbfe_search_for_initialization")
        return n.value, m12, prev


# ------------------------------------------------------------------------------------- Initializer ----
INIT_RESULT_DTYPE = header.dtype("orbfe_init_result")
assert INIT_RESULT_DTYPE.itemsize == 156

_libc_rand = None


def draw_rand_words(count):
    """`count` values of the C library's rand(), seeded once per process with srand(0) -- what DUtils::Random::SeedRandOnce(0) and
    RandomInt do for Initializer::Initialize (Initializer.cc:80-97).  Successive calls continue the same sequence."""
    global _libc_rand
    if _libc_rand is None:
        libc = C.CDLL(None)
        libc.srand.argtypes = [C.c_uint]
        libc.rand.restype = C.c_int
        libc.srand(0)
        _libc_rand = libc.rand
    return np.array([_libc_rand() for _ in range(int(count))], np.int32)


def _init_inputs(kps1, kps2, matches12, K):
    k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
    m12 = np.ascontiguousarray(matches12, np.int32)
    if len(m12) != len(k1):
        raise ValueError("matches12 has %d entries for %d keypoints" % (len(m12), len(k1)))
    K = np.asarray(K, np.float32)
    K4 = np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else K.reshape(4), np.float32)
    return k1, k2, m12, K4


def _ptr_or_none(a):
    return _p(a) if a.size else None


def initialize(kps1, kps2, matches12, K, sigma=1.0, iterations=200, rand_words=None, device=0):
    """Initializer(frame1, sigma, iterations).Initialize(frame2, vMatches12, ...) (Initializer.cc:44-121) on the GPU.
    kps1 / kps2: undistorted keypoints (KP_DTYPE); matches12: len(kps1) ints, -1 = none; K: 3 x 3 or (fx, fy, cx, cy).
    rand_words: iterations * 8 rand() values; None draws them from the C library's rand() seeded once with srand(0).
    Returns (result record of INIT_RESULT_DTYPE, p3d (n1 x 3), triangulated (n1 bools)); the last two are None when the call does
    not initialize (the reference leaves vP3D / vbTriangulated untouched then)."""
    L = load()
    k1, k2, m12, K4 = _init_inputs(kps1, kps2, matches12, K)
    w = draw_rand_words(iterations * 8) if rand_words is None else np.ascontiguousarray(rand_words, np.int32)
    if len(w) != iterations * 8:
        raise ValueError("rand_words needs iterations * 8 = %d values" % (iterations * 8))
    res = np.zeros(1, INIT_RESULT_DTYPE)
    p3d = np.zeros((max(len(k1), 1), 3), np.float32); tri = np.zeros(max(len(k1), 1), np.uint8)
    _check(L, L.orbfe_initialize(_ptr_or_none(k1), len(k1), _ptr_or_none(k2), len(k2), _ptr_or_none(m12), _p(K4), float(sigma),
                                 int(iterations), _p(w), _p(res), _p(p3d), _p(tri), device), "orbfe_initialize")
    if not res[0]["initialized"]:
        return res[0], None, None
    return res[0], p3d[:len(k1)], tri[:len(k1)].astype(bool)


def initialize_inspect(kps1, kps2, matches12, K, sigma=1.0, iterations=200, rand_words=None, device=0):
    """initialize() plus its intermediate results: dict with N, sets (iterations x 8), T1, T2, pn1, pn2, H21 / H12 / F21 of every
    hypothesis (iterations x 3 x 3), SH / SF of every hypothesis, and the result record."""
    L = load()
    k1, k2, m12, K4 = _init_inputs(kps1, kps2, matches12, K)
    w = draw_rand_words(iterations * 8) if rand_words is None else np.ascontiguousarray(rand_words, np.int32)
    res = np.zeros(1, INIT_RESULT_DTYPE)
    n = C.c_int32(0)
    sets = np.zeros((iterations, 8), np.int32); T = np.zeros(18, np.float32)
    pn1 = np.zeros((max(len(k1), 1), 2), np.float32); pn2 = np.zeros((max(len(k2), 1), 2), np.float32)
    models = np.zeros((iterations, 27), np.float32); scores = np.zeros(2 * iterations, np.float32)
    _check(L, L.orbfe_initialize_inspect(_ptr_or_none(k1), len(k1), _ptr_or_none(k2), len(k2), _ptr_or_none(m12), _p(K4), float(sigma),
                                         int(iterations), _p(w), _p(res), C.byref(n), _p(sets), _p(T), _p(pn1), _p(pn2), _p(models),
                                         _p(scores), device), "orbfe_initialize_inspect")
    return dict(N=n.value, sets=sets, T1=T[:9].reshape(3, 3), T2=T[9:].reshape(3, 3), pn1=pn1[:len(k1)], pn2=pn2[:len(k2)],
                H21=models[:, :9].reshape(-1, 3, 3), H12=models[:, 9:18].reshape(-1, 3, 3), F21=models[:, 18:].reshape(-1, 3, 3),
                SH=scores[:iterations], SF=scores[iterations:], result=res[0])


def initialize_check_poses(kps1, kps2, matches12, K, R, t, sigma=1.0, device=0):
    """Initializer::InitializeUseAruco (Initializer.cc:124-189): CheckRT of the given motions R (npose x 3 x 3), t (npose x 3).
    Returns (result record: initialized, best_h = bestIdA, n_good, parallax, R21 / t21; p3d, triangulated) -- the last two None
    when no pose counts a point."""
    L = load()
    k1, k2, m12, K4 = _init_inputs(kps1, kps2, matches12, K)
    R = np.asarray(R, np.float32).reshape(-1, 9); t = np.asarray(t, np.float32).reshape(-1, 3)
    poses = np.ascontiguousarray(np.concatenate([R, t], 1), np.float32)
    res = np.zeros(1, INIT_RESULT_DTYPE)
    p3d = np.zeros((max(len(k1), 1), 3), np.float32); tri = np.zeros(max(len(k1), 1), np.uint8)
    _check(L, L.orbfe_initialize_check_poses(_ptr_or_none(k1), len(k1), _ptr_or_none(k2), len(k2), _ptr_or_none(m12), _p(K4),
                                             float(sigma), _ptr_or_none(poses), len(poses), _p(res), _p(p3d), _p(tri), device),
           "orbfe_initialize_check_poses")
    if res[0]["best_h"] < 0:
        return res[0], None, None
    return res[0], p3d[:len(k1)], tri[:len(k1)].astype(bool)


def initialize_batch_device(d_kps_ptr, d_n_ptr, capacity, npairs, d_matches12_ptr, K, sigma, iterations, d_rand_words_ptr, d_res_ptr,
                            d_p3d_ptr, d_tri_ptr, stream=0):
    """orbfe_initialize_batch_device: pair p = frame p against frame p + 1 of the blocks orbfe_search_for_initialization_batch_device
    reads and writes (device pointers); results: npairs INIT_RESULT_DTYPE records, capacity x 3 p3d and capacity triangulated
    blocks per pair.  Asynchronous on `stream`."""
    L = load()
    K = np.asarray(K, np.float32)
    K4 = np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else K.reshape(4), np.float32)
    _check(L, L.orbfe_initialize_batch_device(d_kps_ptr, d_n_ptr, int(capacity), int(npairs), d_matches12_ptr, _p(K4), float(sigma),
                                              int(iterations), d_rand_words_ptr, d_res_ptr, d_p3d_ptr, d_tri_ptr, stream),
           "orbfe_initialize_batch_device")


# ------------------------------------------------------------------------------- Sim3 RANSAC (loop closing) ----
SIM3_RESULT_DTYPE = header.dtype("orbfe_sim3_result")
assert SIM3_RESULT_DTYPE.itemsize == 148


def _sim3_side(kps, x3Dw, valid, Tcw, K):
    k = np.ascontiguousarray(kps, KP_DTYPE)
    x = np.ascontiguousarray(np.asarray(x3Dw, np.float32).reshape(-1, 3))
    if len(x) != len(k):
        raise ValueError("x3Dw has %d rows for %d keypoints" % (len(x), len(k)))
    v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
    if v is not None and len(v) != len(k):
        raise ValueError("valid has %d entries for %d keypoints" % (len(v), len(k)))
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32)[:3, :4]) if np.ndim(Tcw) == 2 else np.ascontiguousarray(Tcw, np.float32).reshape(3, 4)
    K = np.asarray(K, np.float32)
    K4 = np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else K.reshape(4), np.float32)
    return k, x, v, T, K4


class Sim3Solver:
    """ORB_SLAM2::Sim3Solver (src/Sim3Solver.cc) on the GPU: constructed from the two keyframes' flat arrays and SearchByBoW's
    match12, then iterate(n) / find() as the reference's.  side = (kps (mvKeysUn, KP_DTYPE), x3Dw (n x 3), valid (n, or None), Tcw
    (3 x 4 or 4 x 4), K (3 x 3 or fx, fy, cx, cy)).  The object carries mnIterations, mnBestInliers and the best model; every
    iterate() is one orbfe_sim3_solve call.  rand_words given to iterate() / find(): 3 per iteration of the window, as rand()
    returned them; None draws them with draw_rand_words (the C library's rand(), which DUtils::Random::RandomInt uses)."""

    def __init__(self, side1, side2, match12, level_sigma2, fix_scale=True, device=0):
        self.k1, self.x1, self.v1, self.T1, self.K1 = _sim3_side(*side1)
        self.k2, self.x2, self.v2, self.T2, self.K2 = _sim3_side(*side2)
        if (self.v1 is None) != (self.v2 is None):
            raise ValueError("valid: give both sides or neither")
        self.m12 = np.ascontiguousarray(match12, np.int32)
        if len(self.m12) != len(self.k1):
            raise ValueError("match12 has %d entries for %d keypoints" % (len(self.m12), len(self.k1)))
        self.ls2 = np.ascontiguousarray(level_sigma2, np.float32)
        self.fix_scale = bool(fix_scale)
        self.device = device
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.probability, self.min_inliers, self.max_iterations = float(probability), int(min_inliers), int(max_iterations)
        self.iterations = 0          # mnIterations
        self.best_inliers = 0        # mnBestInliers
        self.s12, self.R12, self.t12, self.T12 = None, None, None, None

    def _args(self, first, n_iterations, best_in, words, res, inl):
        vv = lambda v: None if v is None else _ptr_or_none(v)
        return [_ptr_or_none(self.k1), len(self.k1), _ptr_or_none(self.x1), vv(self.v1), _p(self.T1), _p(self.K1),
                _ptr_or_none(self.k2), len(self.k2), _ptr_or_none(self.x2), vv(self.v2), _p(self.T2), _p(self.K2),
                _ptr_or_none(self.m12), _p(self.ls2), len(self.ls2), int(self.fix_scale), self.probability, self.min_inliers,
                self.max_iterations, int(first), int(n_iterations), int(best_in), _p(words), _p(res), _p(inl)]

    def solve(self, first, n_iterations, best_in, rand_words):
        """One raw orbfe_sim3_solve call, no state kept: (result record, inliers12 as n1 bools)."""
        L = load()
        w = np.ascontiguousarray(rand_words, np.int32)
        if len(w) != 3 * n_iterations:
            raise ValueError("rand_words needs n_iterations * 3 = %d values" % (3 * n_iterations))
        res = np.zeros(1, SIM3_RESULT_DTYPE); inl = np.zeros(max(len(self.k1), 1), np.uint8)
        _check(L, L.orbfe_sim3_solve(*(self._args(first, n_iterations, best_in, w, res, inl) + [self.device])), "orbfe_sim3_solve")
        return res[0], inl[:len(self.k1)].astype(bool)

    def inspect(self, first, n_iterations, best_in, rand_words):
        """solve() plus the intermediate results (orbfe_sim3_inspect): dict with result, inliers12, N, indices1, X3Dc1, X3Dc2, P1im1,
        P2im2, maxError1, maxError2, sets, s12, R12, t12 (per hypothesis) and counts."""
        L = load()
        w = np.ascontiguousarray(rand_words, np.int32)
        n1, it = max(len(self.k1), 1), int(n_iterations)
        res = np.zeros(1, SIM3_RESULT_DTYPE); inl = np.zeros(n1, np.uint8)
        n = C.c_int32(0)
        idx = np.zeros(n1, np.int32); X1 = np.zeros((n1, 3), np.float32); X2 = np.zeros((n1, 3), np.float32)
        P1 = np.zeros((n1, 2), np.float32); P2 = np.zeros((n1, 2), np.float32); e1 = np.zeros(n1, np.float32); e2 = np.zeros(n1, np.float32)
        sets = np.zeros((it, 3), np.int32); models = np.zeros((it, 13), np.float32); counts = np.zeros(it, np.int32)
        _check(L, L.orbfe_sim3_inspect(*(self._args(first, it, best_in, w, res, inl) +
                                         [C.byref(n), _p(idx), _p(X1), _p(X2), _p(P1), _p(P2), _p(e1), _p(e2), _p(sets), _p(models),
                                          _p(counts), self.device])), "orbfe_sim3_inspect")
        N = n.value
        return dict(result=res[0], inliers12=inl[:len(self.k1)].astype(bool), N=N, indices1=idx[:N], X3Dc1=X1[:N], X3Dc2=X2[:N],
                    P1im1=P1[:N], P2im2=P2[:N], maxError1=e1[:N], maxError2=e2[:N], sets=sets, s12=models[:, 0],
                    R12=models[:, 1:10].reshape(-1, 3, 3), t12=models[:, 10:13], counts=counts)

    def iterate(self, n_iterations, rand_words=None):
        """iterate(nIterations, bNoMore, vbInliers, nInliers): returns (T12 4 x 4 or None, no_more, inliers12, n_inliers)."""
        n_iterations = int(n_iterations)
        w = draw_rand_words(3 * n_iterations) if rand_words is None else rand_words
        r, inl = self.solve(self.iterations, n_iterations, self.best_inliers, w)
        if r["best"] >= 0:
            self.best_inliers = int(r["best_inliers"])
            self.s12, self.R12, self.t12 = float(r["s12"]), r["R12"].reshape(3, 3).copy(), r["t12"].copy()
            self.T12 = r["T12"].reshape(4, 4).copy()
        if r["n"] >= self.min_inliers and r["n"] >= 3:
            self.iterations = int(r["found"]) + 1 if r["found"] >= 0 else min(self.iterations + n_iterations, int(r["max_iterations"]))
        self.last = r
        return (self.T12 if r["found"] >= 0 else None), bool(r["no_more"]), inl, int(r["n_inliers"])

    def find(self, rand_words=None):
        """find(vbInliers12, nInliers): (T12 or None, inliers12, n_inliers)."""
        T, _, inl, n = self.iterate(self.max_iterations, rand_words)
        return T, inl, n


def sim3_solve_batch_device(d_kps_ptr, d_n_ptr, capacity, d_x3Dw_ptr, d_valid_ptr, d_Tcw_ptr, d_pair1_ptr, d_pair2_ptr, npairs,
                            d_match12_ptr, K, level_sigma2, fix_scale, probability, min_inliers, max_iterations, d_rand_words_ptr,
                            d_res_ptr, d_inliers12_ptr, stream=0):
    """orbfe_sim3_solve_batch_device: npairs whole runs on the blocks orbfe_search_by_bow_batch_device reads and writes (device
    pointers); results: npairs SIM3_RESULT_DTYPE records and blocks of `capacity` inlier flags.  Asynchronous on `stream`."""
    L = load()
    K = np.asarray(K, np.float32)
    K4 = np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else K.reshape(4), np.float32)
    ls2 = np.ascontiguousarray(level_sigma2, np.float32)
    _check(L, L.orbfe_sim3_solve_batch_device(d_kps_ptr, d_n_ptr, int(capacity), d_x3Dw_ptr, d_valid_ptr, d_Tcw_ptr, d_pair1_ptr,
                                              d_pair2_ptr, int(npairs), d_match12_ptr, _p(K4), _p(ls2), len(ls2), int(bool(fix_scale)),
                                              float(probability), int(min_inliers), int(max_iterations), d_rand_words_ptr, d_res_ptr,
                                              d_inliers12_ptr, stream), "orbfe_sim3_solve_batch_device")


# ------------------------------------------------------------------------------- Sim3 refinement (loop closing) ----
SIM3_OPT_RESULT_DTYPE = header.dtype("orbfe_sim3_opt_result")
assert SIM3_OPT_RESULT_DTYPE.itemsize == 96
SIM3_RESULT_S12_OFFSET = SIM3_RESULT_DTYPE.fields["s12"][1]   # s12, R12, t12: 13 contiguous floats of orbfe_sim3_result


def optimize_sim3(side1, side2, match12, inv_level_sigma2, s12, R12, t12, th2, fix_scale, match12_out=None, device=0):
    """Optimizer::OptimizeSim3 (Optimizer.cc:1544-1739) on the GPU.  side = (kps (mvKeysUn, KP_DTYPE), x3Dw (n x 3), valid (n, or
    None), Tcw (3 x 4 or 4 x 4), K (3 x 3 or fx, fy, cx, cy)) as for Sim3Solver; match12[i1] = i2 or -1; s12, R12 (3 x 3), t12: the
    initial similarity (floats).  match12_out: an int32 array of n1 entries to write (match12 itself works in place; a new array when
    None).  Returns (match12_out, result record of SIM3_OPT_RESULT_DTYPE): n_inliers is the reference's return value, s12 / q12
    (x, y, z, w) / t12 the optimized g2oS12 in double."""
    L = load()
    k1, x1, v1, T1, K1 = _sim3_side(*side1)
    k2, x2, v2, T2, K2 = _sim3_side(*side2)
    if (v1 is None) != (v2 is None):
        raise ValueError("valid: give both sides or neither")
    m12 = match12 if isinstance(match12, np.ndarray) and match12.dtype == np.int32 and match12.flags.c_contiguous else np.ascontiguousarray(match12, np.int32)
    if len(m12) != len(k1):
        raise ValueError("match12 has %d entries for %d keypoints" % (len(m12), len(k1)))
    out = np.full(len(k1), -1, np.int32) if match12_out is None else match12_out
    if out.dtype != np.int32 or len(out) != len(k1) or not out.flags.c_contiguous:
        raise ValueError("match12_out must be a contiguous int32 array of n1 entries")
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    R = np.ascontiguousarray(R12, np.float32).reshape(9)
    t = np.ascontiguousarray(t12, np.float32).reshape(3)
    res = np.zeros(1, SIM3_OPT_RESULT_DTYPE)
    vv = lambda v: None if v is None else _ptr_or_none(v)
    _check(L, L.orbfe_optimize_sim3(_ptr_or_none(k1), len(k1), _ptr_or_none(x1), vv(v1), _p(T1), _p(K1),
                                    _ptr_or_none(k2), len(k2), _ptr_or_none(x2), vv(v2), _p(T2), _p(K2),
                                    _ptr_or_none(m12), _p(sig), len(sig), float(s12), _p(R), _p(t), float(th2), int(bool(fix_scale)),
                                    _ptr_or_none(out), _p(res), device), "orbfe_optimize_sim3")
    return out, res[0]


def optimize_sim3_batch_device(d_kps_ptr, d_n_ptr, capacity, d_x3Dw_ptr, d_valid_ptr, d_Tcw_ptr, d_pair1_ptr, d_pair2_ptr, npairs,
                               d_match12_ptr, K, inv_level_sigma2, d_sim12_ptr, sim12_stride, th2, fix_scale, d_match12_out_ptr,
                               d_res_ptr, stream=0):
    """orbfe_optimize_sim3_batch_device: npairs problems on the blocks orbfe_sim3_solve_batch_device reads (device pointers).
    d_sim12_ptr / sim12_stride: 13 floats s12, R12, t12 per problem (d_res of the Sim3 solver + SIM3_RESULT_S12_OFFSET with its
    itemsize as stride chains the two).  Results: npairs SIM3_OPT_RESULT_DTYPE records, match12_out blocks.  Asynchronous on `stream`."""
    L = load()
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    _check(L, L.orbfe_optimize_sim3_batch_device(d_kps_ptr, d_n_ptr, int(capacity), d_x3Dw_ptr, d_valid_ptr, d_Tcw_ptr, d_pair1_ptr,
                                                 d_pair2_ptr, int(npairs), d_match12_ptr, _p(_K4(K)), _p(sig), len(sig), d_sim12_ptr,
                                                 int(sim12_stride), float(th2), int(bool(fix_scale)), d_match12_out_ptr, d_res_ptr,
                                                 stream), "orbfe_optimize_sim3_batch_device")


# ------------------------------------------------------------------------------- KeyFrameDatabase queries ----
KFDB_LOOP, KFDB_RELOC, KFDB_NEIGHBOURS, KFDB_MAX_KEYFRAMES, KFDB_MAX_WORDS = _defines(
    "KFDB_LOOP", "KFDB_RELOC", "KFDB_NEIGHBOURS", "KFDB_MAX_KEYFRAMES", "KFDB_MAX_WORDS")
L1_NORM = 0   # DBoW2::ScoringType
KFDB_RESULT_DTYPE = header.dtype("orbfe_kfdb_result")
assert KFDB_RESULT_DTYPE.itemsize == 36


def _bow_csr(offsets, word, value):
    return np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(word, np.uint32), np.ascontiguousarray(value, np.float64)


def detect_candidates(mode, q_word, q_value, offsets, word, value, neigh, scores, active=None, connected=None, min_score=0.0,
                      scoring=L1_NORM, device=0):
    """KeyFrameDatabase::DetectLoopCandidates (mode KFDB_LOOP) / DetectRelocalizationCandidates (KFDB_RELOC) on the GPU.  Query
    BowVector q_word (ascending) / q_value; database of K keyframes in add order as CSR offsets / word / value, active (K flags or
    None), neigh (K x 10 positions, negative = none); loop mode: connected positions and min_score.  scores: float32 array of K
    entries, the mLoopScore / mRelocScore state, UPDATED IN PLACE.  Returns (candidates, common (K counts), record of
    KFDB_RESULT_DTYPE)."""
    L = load()
    off, w, v = _bow_csr(offsets, word, value)
    K = len(off) - 1
    qw, qv = np.ascontiguousarray(q_word, np.uint32), np.ascontiguousarray(q_value, np.float64)
    ng = np.ascontiguousarray(neigh, np.int32).reshape(K, KFDB_NEIGHBOURS)
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    conn = np.zeros(0, np.int32) if connected is None else np.ascontiguousarray(connected, np.int32)
    if not (isinstance(scores, np.ndarray) and scores.dtype == np.float32 and scores.flags.c_contiguous and len(scores) == K):
        raise ValueError("scores must be a contiguous float32 array of K entries")
    cand, common, res = np.full(K, -1, np.int32), np.zeros(K, np.int32), np.zeros(1, KFDB_RESULT_DTYPE)
    _check(L, L.orbfe_detect_candidates(int(mode), int(scoring), _ptr_or_none(qw), _ptr_or_none(qv), len(qw), _p(off), _ptr_or_none(w),
                                        _ptr_or_none(v), None if act is None else _ptr_or_none(act), K, _ptr_or_none(ng),
                                        _ptr_or_none(conn), len(conn), float(min_score), _ptr_or_none(scores), _ptr_or_none(cand),
                                        _ptr_or_none(common), _p(res), device), "orbfe_detect_candidates")
    return cand[:res[0]["n_candidates"]].copy(), common, res[0]


def detect_candidates_batch_device(mode, d_bow_word_ptr, d_bow_value_ptr, d_nbow_ptr, capacity, d_db_ptr, d_active_ptr, K, d_query_ptr, nq,
                                   d_neigh_ptr, d_conn_offsets_ptr, d_conn_ptr, d_min_score_ptr, d_scores_ptr, d_candidates_ptr,
                                   d_common_ptr, d_scratch_ptr, d_res_ptr, stream=0, scoring=L1_NORM):
    """orbfe_detect_candidates_batch_device: nq queries against K resident keyframes in the block layout of
    orbfe_vocabulary_transform_batch_device (device pointers; see include/orbfe.h).  Asynchronous on `stream`."""
    L = load()
    _check(L, L.orbfe_detect_candidates_batch_device(int(mode), int(scoring), d_bow_word_ptr, d_bow_value_ptr, d_nbow_ptr, int(capacity),
                                                     d_db_ptr, d_active_ptr, int(K), d_query_ptr, int(nq), d_neigh_ptr, d_conn_offsets_ptr,
                                                     d_conn_ptr, d_min_score_ptr, d_scores_ptr, d_candidates_ptr, d_common_ptr,
                                                     d_scratch_ptr, d_res_ptr, stream), "orbfe_detect_candidates_batch_device")


def bow_min_score_batch_device(d_bow_word_ptr, d_bow_value_ptr, d_nbow_ptr, capacity, d_db_ptr, d_active_ptr, K, d_query_ptr, nq,
                               d_conn_offsets_ptr, d_conn_ptr, d_min_score_ptr, stream=0, scoring=L1_NORM):
    """orbfe_bow_min_score_batch_device: DetectLoop's minScore per query into d_min_score (device pointers)."""
    L = load()
    _check(L, L.orbfe_bow_min_score_batch_device(int(scoring), d_bow_word_ptr, d_bow_value_ptr, d_nbow_ptr, int(capacity), d_db_ptr,
                                                 d_active_ptr, int(K), d_query_ptr, int(nq), d_conn_offsets_ptr, d_conn_ptr,
                                                 d_min_score_ptr, stream), "orbfe_bow_min_score_batch_device")


def bow_score(offsets, word, value, pair1, pair2, scoring=L1_NORM, device=0):
    """(float)L1Scoring::score of the BowVector pairs (pair1[p], pair2[p]) of a CSR set, on the GPU."""
    L = load()
    off, w, v = _bow_csr(offsets, word, value)
    p1, p2 = np.ascontiguousarray(pair1, np.int32), np.ascontiguousarray(pair2, np.int32)
    out = np.zeros(len(p1), np.float32)
    _check(L, L.orbfe_bow_score(int(scoring), _p(off), _ptr_or_none(w), _ptr_or_none(v), len(off) - 1, _ptr_or_none(p1), _ptr_or_none(p2),
                                len(p1), _ptr_or_none(out), device), "orbfe_bow_score")
    return out


def bow_score_batch_device(d_bow_word_ptr, d_bow_value_ptr, d_nbow_ptr, capacity, d_pair1_ptr, d_pair2_ptr, npairs, d_scores_ptr, stream=0,
                           scoring=L1_NORM):
    """orbfe_bow_score_batch_device: the same on the block layout (device pointers)."""
    L = load()
    _check(L, L.orbfe_bow_score_batch_device(int(scoring), d_bow_word_ptr, d_bow_value_ptr, d_nbow_ptr, int(capacity), d_pair1_ptr,
                                             d_pair2_ptr, int(npairs), d_scores_ptr, stream), "orbfe_bow_score_batch_device")


# ------------------------------------------------------------------------------- pose optimization ----
POSE_MARKER_DTYPE = header.dtype("orbfe_pose_marker")
POSE_RESULT_DTYPE = header.dtype("orbfe_pose_result")
assert POSE_MARKER_DTYPE.itemsize == 128 and POSE_RESULT_DTYPE.itemsize == 56


def _K4(K):
    K = np.asarray(K, np.float32)
    return np.ascontiguousarray([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else K.reshape(4), np.float32)


def pose_optimization(kps, has_mp, x3Dw, inv_level_sigma2, K, Tcw, markers=None, marker_info=25.0, outlier=None, device=0):
    """Optimizer::PoseOptimizationByAruco (Optimizer.cc:522-770) on the GPU; markers=None (or empty) is PoseOptimization without
    its stereo branch.  kps: undistorted keypoints (KP_DTYPE); has_mp: n flags; x3Dw: n x 3 world points; inv_level_sigma2:
    mvInvLevelSigma2; K: 3 x 3 or (fx, fy, cx, cy); Tcw: 3 x 4 [R | t]; markers: POSE_MARKER_DTYPE records.  outlier: n uint8 updated
    in place where has_mp (a new zero array when None).  Returns (Tcw_out 3 x 4, outlier, chi2 (n floats: the last classification's,
    NaN where not written), result record of POSE_RESULT_DTYPE)."""
    L = load()
    k = np.ascontiguousarray(kps, KP_DTYPE)
    n = len(k)
    has = np.ascontiguousarray(has_mp, np.uint8)
    X = np.ascontiguousarray(x3Dw, np.float32).reshape(-1, 3)
    if len(has) != n or len(X) != n:
        raise ValueError("has_mp / x3Dw need one entry per keypoint")
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    mk = np.ascontiguousarray(np.zeros(0, POSE_MARKER_DTYPE) if markers is None else markers, POSE_MARKER_DTYPE)
    T_in = np.ascontiguousarray(Tcw, np.float32).reshape(12)
    T_out = np.zeros(12, np.float32)
    out = np.zeros(n, np.uint8) if outlier is None else outlier
    if out.dtype != np.uint8 or len(out) != n or not out.flags.c_contiguous:
        raise ValueError("outlier must be a contiguous uint8 array of n entries")
    chi2 = np.full(n, np.nan, np.float32)
    res = np.zeros(1, POSE_RESULT_DTYPE)
    _check(L, L.orbfe_pose_optimization(_ptr_or_none(k), n, _ptr_or_none(has), _ptr_or_none(X), _p(sig), len(sig), _p(_K4(K)),
                                        _ptr_or_none(mk), len(mk), float(marker_info), _p(T_in), _p(T_out), _ptr_or_none(out),
                                        _ptr_or_none(chi2), _p(res), device), "orbfe_pose_optimization")
    return T_out.reshape(3, 4), out, chi2, res[0]


def pose_optimization_batch_device(d_kps_ptr, d_n_ptr, capacity, nframes, d_has_mp_ptr, d_x3Dw_ptr, d_markers_ptr, d_nm_ptr, mcapacity,
                                   inv_level_sigma2, K, marker_info, d_Tcw_in_ptr, d_Tcw_out_ptr, d_outlier_ptr, d_chi2_ptr, d_res_ptr,
                                   stream=0):
    """orbfe_pose_optimization_batch_device over nframes problems in `capacity` / `mcapacity` blocks (device pointers; d_markers /
    d_nm / d_chi2 may be None).  Asynchronous on `stream`."""
    L = load()
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    _check(L, L.orbfe_pose_optimization_batch_device(d_kps_ptr, d_n_ptr, int(capacity), int(nframes), d_has_mp_ptr, d_x3Dw_ptr,
                                                     d_markers_ptr, d_nm_ptr, int(mcapacity), _p(sig), len(sig), _p(_K4(K)),
                                                     float(marker_info), d_Tcw_in_ptr, d_Tcw_out_ptr, d_outlier_ptr, d_chi2_ptr,
                                                     d_res_ptr, stream), "orbfe_pose_optimization_batch_device")


def pose_gather_device(d_match_cur_ptr, d_n_ptr, capacity, nframes, d_q_x3Dw_ptr, d_nq_ptr, qcapacity, d_has_mp_ptr, d_x3Dw_ptr, stream=0):
    """orbfe_pose_gather_device: has_mp / x3Dw blocks from mode 2's match_cur and the queries' world points (device pointers)."""
    L = load()
    _check(L, L.orbfe_pose_gather_device(d_match_cur_ptr, d_n_ptr, int(capacity), int(nframes), d_q_x3Dw_ptr, d_nq_ptr, int(qcapacity),
                                         d_has_mp_ptr, d_x3Dw_ptr, stream), "orbfe_pose_gather_device")


# ------------------------------------------------------------------------------------------ ArUco ----
RECT_DTYPE = np.dtype([("corners", "<f4", (4, 2)), ("off", "<i4"), ("len", "<i4")])


def camera_resize(K, cam_size, img_size):
    """CameraParameters::resize (cameraparameters.cpp:158-173); sizes are (width, height)."""
    L = load()
    K4, _ = _camera(K, None)
    out = np.zeros(4, np.float32)
    _check(L, L.orbfe_camera_resize(_p(K4), int(cam_size[0]), int(cam_size[1]), int(img_size[0]), int(img_size[1]), _p(out)),
           "orbfe_camera_resize")
    return out


def marker_poses(markers, marker_size, K, dist, device=0):
    """Both IPPE poses + reprojection errors of every marker (marker.cpp:322-344, ippe.cpp:72-100, Frame.cc:170-174)."""
    L = load()
    K4, d = _camera(K, dist)
    mk = np.ascontiguousarray(markers, MARKER_DTYPE)
    out = np.zeros(len(mk), POSE_DTYPE)
    _check(L, L.orbfe_marker_poses(_p(mk), len(mk), marker_size, _p(K4), _p(d) if len(d) else None, len(d), _p(out), device),
           "orbfe_marker_poses")
    return out


def search_by_bow(kps1, desc1, fv1, kps2, desc2, fv2, valid1=None, valid2=None, nnratio=0.7, check_orientation=True,
                  accept_max=50, factor=30 / 360.0, device=0):
    """ORBmatcher::SearchByBoW on flat arrays (ORBmatcher.cc:159-292; :526-659 with valid2, accept_max=49, factor=1/30).
    fv = (node ids, offsets, feature indices) as ORBVocabulary.transform returns.  -> (nmatches, match12, match21)."""
    L = load()
    k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
    d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    a = [np.ascontiguousarray(fv1[0], np.uint32), np.ascontiguousarray(fv1[1], np.int32), np.ascontiguousarray(fv1[2], np.uint32)]
    b = [np.ascontiguousarray(fv2[0], np.uint32), np.ascontiguousarray(fv2[1], np.int32), np.ascontiguousarray(fv2[2], np.uint32)]
    v1 = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8)
    v2 = None if valid2 is None else np.ascontiguousarray(valid2, np.uint8)
    m12 = np.full(len(k1), -1, np.int32); m21 = np.full(len(k2), -1, np.int32); nm = C.c_int32(0)
    _check(L, L.orbfe_search_by_bow(_p(k1), _p(d1), None if v1 is None else _p(v1), len(k1), _p(a[0]), _p(a[1]), _p(a[2]), len(a[0]),
                                    _p(k2), _p(d2), None if v2 is None else _p(v2), len(k2), _p(b[0]), _p(b[1]), _p(b[2]), len(b[0]),
                                    nnratio, int(check_orientation), accept_max, np.float32(factor), _p(m12), _p(m21), C.byref(nm),
                                    device), "orbfe_search_by_bow")
    return nm.value, m12, m21


KF_FEATURE_BYTES = header.defines["KF_FEATURE_BYTES"]


def keyframe_features_pack(kps, desc, mp_index=None, device=0):
    """Feature records of Map::SaveKeyFrame (Map.cc:297-321) -> bytes (n x 68)."""
    L = load()
    k = np.ascontiguousarray(kps, KP_DTYPE); d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    m = None if mp_index is None else np.ascontiguousarray(mp_index, np.uint64)
    out = np.zeros(len(k) * KF_FEATURE_BYTES, np.uint8)
    _check(L, L.orbfe_keyframe_features_pack(_p(k), _p(d), None if m is None else _p(m), len(k), _p(out), device),
           "orbfe_keyframe_features_pack")
    return out


def keyframe_features_unpack(buf, n, device=0):
    """The read side (Map::LoadKeyFrame, Map.cc:478-511) -> (keypoints, descriptors, map point indices)."""
    L = load()
    b = np.ascontiguousarray(buf, np.uint8)
    assert len(b) >= n * KF_FEATURE_BYTES
    k = np.zeros(n, KP_DTYPE); d = np.zeros((n, 32), np.uint8); m = np.zeros(n, np.uint64)
    _check(L, L.orbfe_keyframe_features_unpack(_p(b), n, _p(k), _p(d), _p(m), device), "orbfe_keyframe_features_unpack")
    return k, d, m


def search_for_triangulation(kps1, desc1, fv1, kps2, desc2, fv2, F12, epipole, scale_factors, level_sigma2, has_mp1=None, has_mp2=None,
                             check_orientation=True, device=0):
    """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:661-827, mono) -> (nmatches, match12)."""
    L = load()
    k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
    d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    a = [np.ascontiguousarray(fv1[0], np.uint32), np.ascontiguousarray(fv1[1], np.int32), np.ascontiguousarray(fv1[2], np.uint32)]
    b = [np.ascontiguousarray(fv2[0], np.uint32), np.ascontiguousarray(fv2[1], np.int32), np.ascontiguousarray(fv2[2], np.uint32)]
    h1 = None if has_mp1 is None else np.ascontiguousarray(has_mp1, np.uint8)
    h2 = None if has_mp2 is None else np.ascontiguousarray(has_mp2, np.uint8)
    F = np.ascontiguousarray(F12, np.float32).reshape(9); sf = np.ascontiguousarray(scale_factors, np.float32)
    sg = np.ascontiguousarray(level_sigma2, np.float32)
    m12 = np.full(len(k1), -1, np.int32); nm = C.c_int32(0)
    _check(L, L.orbfe_search_for_triangulation(_p(k1), _p(d1), None if h1 is None else _p(h1), len(k1), _p(a[0]), _p(a[1]), _p(a[2]), len(a[0]),
                                               _p(k2), _p(d2), None if h2 is None else _p(h2), len(k2), _p(b[0]), _p(b[1]), _p(b[2]), len(b[0]),
                                               _p(F), np.float32(epipole[0]), np.float32(epipole[1]), _p(sf), _p(sg), len(sf),
                                               int(check_orientation), _p(m12), C.byref(nm), device), "orbfe_search_for_triangulation")
    return nm.value, m12


NEW_POINTS_PAIR_DTYPE = header.dtype("orbfe_new_points_pair")
NEW_POINTS_RESULT_DTYPE = header.dtype("orbfe_new_points_result")
NMP_CREATED = header.defines["NMP_CREATED"]


def _tcw12(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(-1, 4)[:3], np.float32).reshape(12)


def _new_points_keyframe(kf):
    """a keyframe of create_new_map_points as contiguous arrays: kps, desc, fv (node, offset, feature), x3Dw, valid, Tcw"""
    k = np.ascontiguousarray(kf["kps"], KP_DTYPE)
    d = np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32)
    fv = [np.ascontiguousarray(kf["fv"][0], np.uint32), np.ascontiguousarray(kf["fv"][1], np.int32), np.ascontiguousarray(kf["fv"][2], np.uint32)]
    x = np.array(kf["x3Dw"], np.float32).reshape(-1, 3)
    v = (np.asarray(kf["valid"]).reshape(-1) != 0).astype(np.uint8)
    if not (len(k) == len(d) == len(x) == len(v)):
        raise ValueError("a keyframe's arrays differ in length")
    return dict(kps=k, desc=d, fv=fv, x3Dw=x, valid=v, Tcw=_tcw12(kf["Tcw"]))


def create_new_map_points(cur, neighbours, K, scale_factors, level_sigma2, ratio_factor=None, check_orientation=False, device=0):
    """LocalMapping::CreateNewMapPoints (LocalMapping.cc:222-467, monocular) of the keyframe `cur` against `neighbours`, in list
    order.  A keyframe is a dict: kps (mvKeysUn, KP_DTYPE), desc (n x 32), fv (node, offset, feature: the FeatureVector), x3Dw
    (n x 3), valid (n; has a map point), Tcw (3 x 4 or 4 x 4).  K: 3 x 3 or fx, fy, cx, cy.  ratio_factor defaults to
    1.5f * scale_factors[1].  The inputs are not changed.  Returns (list with one dict per neighbour: i1, i2, x3D, normal,
    max_distance, min_distance of the created points in ascending i1, status (n1 bytes), match12, F12, epipole, prep, result;
    the current keyframe's (x3Dw, valid) after the last neighbour)."""
    L = load()
    c = _new_points_keyframe(cur)
    Kf = np.asarray(K, np.float32)
    K4 = np.ascontiguousarray([Kf[0, 0], Kf[1, 1], Kf[0, 2], Kf[1, 2]] if Kf.size == 9 else Kf.reshape(4), np.float32)
    sf = np.ascontiguousarray(scale_factors, np.float32); sg = np.ascontiguousarray(level_sigma2, np.float32)
    if len(sf) != len(sg):
        raise ValueError("scale_factors and level_sigma2 differ in length")
    rf = float(np.float32(1.5) * sf[min(1, len(sf) - 1)]) if ratio_factor is None else float(ratio_factor)
    n1 = len(c["kps"])
    out = []
    for nb in neighbours:
        b = _new_points_keyframe(nb)
        F12 = np.zeros(9, np.float32); ep = np.zeros(2, np.float32)
        prep = np.zeros(1, NEW_POINTS_PAIR_DTYPE); res = np.zeros(1, NEW_POINTS_RESULT_DTYPE)
        m12 = np.full(n1, -1, np.int32); status = np.zeros(n1, np.uint8)
        x3D = np.zeros((n1, 3), np.float32); normal = np.zeros((n1, 3), np.float32); dist = np.zeros((n1, 2), np.float32)
        side = lambda f: [_ptr_or_none(f["kps"]), _ptr_or_none(f["desc"]), len(f["kps"]), _ptr_or_none(f["fv"][0]), _ptr_or_none(f["fv"][1]),
                          _ptr_or_none(f["fv"][2]), len(f["fv"][0]), _ptr_or_none(f["x3Dw"]), _ptr_or_none(f["valid"]), _p(f["Tcw"])]
        _check(L, L.orbfe_create_new_map_points(*(side(c) + side(b) + [_p(K4), _p(sf), _p(sg), len(sf), rf, int(bool(check_orientation)),
                                                                        _p(F12), _p(ep), _p(prep), _ptr_or_none(m12), _ptr_or_none(status),
                                                                        _ptr_or_none(x3D), _ptr_or_none(normal), _ptr_or_none(dist), _p(res), device])),
               "orbfe_create_new_map_points")
        i1 = np.flatnonzero(status == NMP_CREATED)
        out.append(dict(i1=i1, i2=m12[i1], x3D=x3D[i1], normal=normal[i1], max_distance=dist[i1, 0], min_distance=dist[i1, 1], status=status,
                        match12=m12, F12=F12.reshape(3, 3), epipole=ep, prep=prep[0], result=res[0], x3Dw2=b["x3Dw"], valid2=b["valid"]))
    return out, (c["x3Dw"], c["valid"])


def new_points_inspect(kps1, Tcw1, kps2, Tcw2, match12, K4, scale_factors, level_sigma2, ratio_factor, device=0):
    """orbfe_new_points_inspect (diagnostic): the triangulation of a given match list with its gate quantities ->
    dict(status, x3D, normal, dist, quantities (n1 x 6: cos, err1, err2, dist1, dist2, ratioOctave), result)."""
    L = load()
    k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
    m12 = np.ascontiguousarray(match12, np.int32)
    if len(m12) != len(k1):
        raise ValueError("match12 has %d entries for %d keypoints" % (len(m12), len(k1)))
    sf = np.ascontiguousarray(scale_factors, np.float32); sg = np.ascontiguousarray(level_sigma2, np.float32)
    K = np.ascontiguousarray(K4, np.float32).reshape(4)
    n1 = len(k1)
    status = np.zeros(n1, np.uint8); x3D = np.zeros((n1, 3), np.float32); normal = np.zeros((n1, 3), np.float32)
    dist = np.zeros((n1, 2), np.float32); q = np.zeros((n1, 6), np.float32); res = np.zeros(1, NEW_POINTS_RESULT_DTYPE)
    _check(L, L.orbfe_new_points_inspect(_ptr_or_none(k1), n1, _p(_tcw12(Tcw1)), _ptr_or_none(k2), len(k2), _p(_tcw12(Tcw2)), _ptr_or_none(m12),
                                         _p(K), _p(sf), _p(sg), len(sf), float(ratio_factor), _ptr_or_none(status), _ptr_or_none(x3D),
                                         _ptr_or_none(normal), _ptr_or_none(dist), _ptr_or_none(q), _p(res), device), "orbfe_new_points_inspect")
    return dict(status=status, x3D=x3D, normal=normal, dist=dist, quantities=q, result=res[0])


class ORBVocabulary:
    """Mirror of ORB_SLAM2::ORBVocabulary (include/ORBVocabulary.h: DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) for
    the per-frame path: loadFromTextFile + transform(features, BowVector, FeatureVector, levelsup)."""

    def __init__(self, device=0):
        self.L = load()
        self.h = None
        self.device = device

    def __del__(self):
        if getattr(self, "h", None):
            self.L.orbfe_vocabulary_destroy(self.h)
            self.h = None

    def loadFromTextFile(self, filename):
        if self.h:
            self.L.orbfe_vocabulary_destroy(self.h)
        self.h = self.L.orbfe_vocabulary_load_text(os.fsencode(filename), self.device)
        if not self.h:
            raise OrbfeError("orbfe_vocabulary_load_text: " + self.L.orbfe_last_error().decode())
        return True

    @classmethod
    def from_arrays(cls, k, L, scoring, weighting, parent, is_leaf, descriptors, weights, device=0):
        self = cls(device)
        parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        descriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        weights = np.ascontiguousarray(weights, np.float64)
        self.h = self.L.orbfe_vocabulary_create(k, L, scoring, weighting, len(parent), _p(parent), _p(is_leaf), _p(descriptors),
                                                _p(weights), device)
        if not self.h:
            raise OrbfeError("orbfe_vocabulary_create: " + self.L.orbfe_last_error().decode())
        return self

    def info(self):
        out = np.zeros(6, np.int32)
        _check(self.L, self.L.orbfe_vocabulary_info(self.h, _p(out)), "orbfe_vocabulary_info")
        return dict(zip(("k", "L", "scoring", "weighting", "nodes", "words"), out.tolist()))

    def transform(self, descriptors, levelsup=4):
        """-> dict(word, node, weight per feature; bow = (word ids, values); fv = (node ids, offsets, feature indices))"""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        word = np.zeros(n, np.int32); node = np.zeros(n, np.int32); weight = np.zeros(n, np.float64)
        bw = np.zeros(n, np.uint32); bv = np.zeros(n, np.float64); fn = np.zeros(n, np.uint32)
        fo = np.zeros(n + 1, np.int32); ff = np.zeros(n, np.uint32)
        nb, nf = C.c_int32(0), C.c_int32(0)
        _check(self.L, self.L.orbfe_vocabulary_transform(self.h, _p(d), n, levelsup, _p(word), _p(node), _p(weight), _p(bw), _p(bv),
                                                         C.byref(nb), _p(fn), _p(fo), _p(ff), C.byref(nf)),
               "orbfe_vocabulary_transform")
        nb, nf = nb.value, nf.value
        return dict(word=word, node=node, weight=weight, bow=(bw[:nb].copy(), bv[:nb].copy()),
                    fv=(fn[:nf].copy(), fo[:nf + 1].copy(), ff[:fo[nf]].copy()))


def corner_subpix(image, pts, win, max_iters, eps, device=0):
    """cv::cornerSubPix(image, pts, Size(win, win), Size(-1, -1), TermCriteria(MAX_ITER | EPS, max_iters, eps)) -> refined (n, 2) float32."""
    L = load()
    image = np.ascontiguousarray(image, np.uint8)
    out = np.ascontiguousarray(pts, np.float32).reshape(-1, 2).copy()
    _check(L, L.orbfe_corner_subpix(_p(image), image.shape[0], image.shape[1], image.strides[0], _p(out), len(out), int(win), int(max_iters),
                                    float(eps), device), "orbfe_corner_subpix")
    return out


class MarkerDetector:
    """Mirror of aruco::MarkerDetector as the reference configures it (src/Frame.cc:129-142):
    setDictionary(name) + DM_NORMAL + CORNER_LINES; detect(image) -> markers sorted by id."""
    # order of kernel_times_us(); the pyramid runs on the detector's second stream, concurrently with threshold + contours
    STAGES = ["pyramid", "threshold", "contours", "decode", "finalize"]

    def __init__(self, dictionary="ARUCO", device=0):
        self.L = load()
        self.h = self.L.orbfe_aruco_create(dictionary.encode(), device)
        if not self.h:
            raise OrbfeError("orbfe_aruco_create: " + self.L.orbfe_last_error().decode())
        self.capacity = self.L.orbfe_aruco_max_markers(self.h)
        self._shape = None

    @classmethod
    def wrap(cls, handle):
        """A non-owning view of a detector another object owns (the detector of an orbfe_pipeline)."""
        self = cls.__new__(cls)
        self.L = load()
        self.h = handle
        self._borrowed = True
        self.capacity = self.L.orbfe_aruco_max_markers(self.h)
        self._shape = None
        return self

    def __del__(self):
        if getattr(self, "h", None) and not getattr(self, "_borrowed", False):
            self.L.orbfe_aruco_destroy(self.h)
        self.h = None

    DM_NORMAL, DM_FAST, DM_VIDEO_FAST = 0, 1, 2              # aruco::DetectionMode (markerdetector.h:60)
    CORNER_SUBPIX, CORNER_LINES, CORNER_NONE = 0, 1, 2       # aruco::CornerRefinementMethod (:62)

    def setDictionary(self, name, error_correction_rate=0.0):
        _check(self.L, self.L.orbfe_aruco_set_dictionary(self.h, name.encode()), "orbfe_aruco_set_dictionary")
        _check(self.L, self.L.orbfe_aruco_set_error_correction_rate(self.h, error_correction_rate), "orbfe_aruco_set_error_correction_rate")

    def setDetectionMode(self, dm, minMarkerSize=0.0):
        _check(self.L, self.L.orbfe_aruco_set_detection_mode(self.h, int(dm), minMarkerSize), "orbfe_aruco_set_detection_mode")

    def setCornerRefinementMethod(self, method):
        _check(self.L, self.L.orbfe_aruco_set_corner_refinement(self.h, int(method)), "orbfe_aruco_set_corner_refinement")

    def detectEnclosedMarkers(self, on=True):
        """Params::detectEnclosedMarkers (markerdetector.h:126)."""
        _check(self.L, self.L.orbfe_aruco_set_enclosed_markers(self.h, int(on)), "orbfe_aruco_set_enclosed_markers")

    def setTracking(self, min_detections):
        """Params::trackingMinDetections (markerdetector.h:187); resets the history."""
        _check(self.L, self.L.orbfe_aruco_set_tracking(self.h, int(min_detections)), "orbfe_aruco_set_tracking")

    def tracked(self):
        return self.L.orbfe_aruco_last_tracked(self.h)

    def setGrayConversion(self, fractional_bits):
        """cvtColor(BGR2GRAY) of CV_8UC3 frames: 14 fractional bits (OpenCV <= 3.4.1, default) or 15 (3.4.2 and later)."""
        _check(self.L, self.L.orbfe_aruco_set_gray_conversion(self.h, int(fractional_bits)), "orbfe_aruco_set_gray_conversion")

    def state(self):
        """Params::ThresHold and Params::minSize as the last call left them, its threshold passes and working image size."""
        t, a, r, c, m = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_float(0)
        _check(self.L, self.L.orbfe_aruco_get_state(self.h, C.byref(t), C.byref(m), C.byref(a), C.byref(r), C.byref(c)), "orbfe_aruco_get_state")
        return {"threshold": t.value, "min_size": m.value, "attempts": a.value, "work_shape": (r.value, c.value)}

    def contour(self, marker, frame=0):
        """aruco::Marker::contourPoints of output marker `marker` of the last call -> (n, 2) int32."""
        n = C.c_int32(0)
        _check(self.L, self.L.orbfe_aruco_marker_contour(self.h, frame, marker, None, 0, C.byref(n)), "orbfe_aruco_marker_contour")
        xy = np.zeros((max(n.value, 1), 2), np.int32)
        _check(self.L, self.L.orbfe_aruco_marker_contour(self.h, frame, marker, _p(xy), n.value, C.byref(n)), "orbfe_aruco_marker_contour")
        return xy[:n.value]

    def contours(self, nmarkers, frame=0):
        """contourPoints of the first `nmarkers` output markers of `frame` in one round trip -> list of (n, 2) int32."""
        off = np.zeros(nmarkers + 1, np.int32)
        _check(self.L, self.L.orbfe_aruco_marker_contours(self.h, frame, nmarkers, None, 0, _p(off)), "orbfe_aruco_marker_contours")
        xy = np.zeros((max(int(off[-1]), 1), 2), np.int32)
        _check(self.L, self.L.orbfe_aruco_marker_contours(self.h, frame, nmarkers, _p(xy), int(off[-1]), _p(off)), "orbfe_aruco_marker_contours")
        return [xy[off[i]:off[i + 1]] for i in range(nmarkers)]

    def detect(self, image, camera=None, markerSizeMeters=-1.0):
        """detect(image) -> MARKER_DTYPE records.  With camera = (K, dist, (cam_width, cam_height)) and a marker size
        (markerdetector.h:276-312; Frame.cc:142 passes 0.187) -> (markers, POSE_DTYPE poses): the camera matrix is
        rescaled to the image size first (markerdetector_impl.cpp:1110-1172), then every marker gets its IPPE pose."""
        if camera is not None and markerSizeMeters > 0:
            K, dist, cam_size = camera
            K4, d = _camera(K, dist)
            image = np.asarray(image)
            if image.size == 0:
                return np.zeros(0, MARKER_DTYPE), np.zeros(0, POSE_DTYPE)
            bgr = image.ndim == 3 and image.shape[2] == 3   # CV_8UC3: cvtColor(BGR2GRAY) first (markerdetector_impl.cpp:5892)
            assert image.dtype == np.uint8 and (image.ndim == 2 or bgr)
            if image.strides[1] != (3 if bgr else 1) or (bgr and image.strides[2] != 1):
                image = np.ascontiguousarray(image)
            rows, cols = image.shape[:2]
            K4 = np.ascontiguousarray(camera_resize(K4, cam_size, (cols, rows)), np.float32)
            out = np.zeros(self.capacity, MARKER_DTYPE)
            poses = np.zeros(self.capacity, POSE_DTYPE)
            n = C.c_int32(0)
            fn = self.L.orbfe_aruco_detect_poses_bgr if bgr else self.L.orbfe_aruco_detect_poses
            _check(self.L, fn(self.h, _p(image), rows, cols, image.strides[0], _p(out), _p(poses), self.capacity,
                                                           C.byref(n), markerSizeMeters, _p(K4), _p(d) if d is not None and len(d) else None,
                                                           0 if d is None else len(d)), "orbfe_aruco_detect_poses")
            self._shape = image.shape[:2]
            return out[:n.value].copy(), poses[:n.value].copy()
        image = np.asarray(image)
        if image.size == 0:
            return np.zeros(0, MARKER_DTYPE)
        bgr = image.ndim == 3 and image.shape[2] == 3
        assert image.dtype == np.uint8 and (image.ndim == 2 or bgr)
        if image.strides[1] != (3 if bgr else 1) or (bgr and image.strides[2] != 1):
            image = np.ascontiguousarray(image)
        out = np.zeros(self.capacity, MARKER_DTYPE)
        n = C.c_int32(0)
        fn = self.L.orbfe_aruco_detect_bgr if bgr else self.L.orbfe_aruco_detect
        _check(self.L, fn(self.h, _p(image), image.shape[0], image.shape[1], image.strides[0],
                          _p(out), self.capacity, C.byref(n)), "orbfe_aruco_detect")
        self._shape = image.shape[:2]
        return out[:n.value].copy()

    def detect_batch(self, images):
        images = np.ascontiguousarray(images, np.uint8)
        B, rows, cols = images.shape
        out = np.zeros((B, self.capacity), MARKER_DTYPE)
        n = np.zeros(B, np.int32)
        _check(self.L, self.L.orbfe_aruco_detect_batch(self.h, _p(images), B, images.strides[0], rows, cols,
                                                       images.strides[1], _p(out), self.capacity, _p(n)),
               "orbfe_aruco_detect_batch")
        self._shape = (rows, cols)
        return [out[f, :n[f]].copy() for f in range(B)]

    def detect_batch_device(self, d_imgs_ptr, B, frame_stride, rows, cols, step, d_out_ptr, capacity, d_n_ptr,
                            stream=0):
        _check(self.L, self.L.orbfe_aruco_detect_batch_device(self.h, d_imgs_ptr, B, frame_stride, rows, cols, step,
                                                              d_out_ptr, capacity, d_n_ptr, stream),
               "orbfe_aruco_detect_batch_device")
        self._shape = (rows, cols)

    def batch_status(self):
        """(frames of the last device batch with incomplete results, union of their capacity flags; ARUCO_FLAG_TRUNCATED: the
        caller's capacity was too small, repeat with up to self.capacity records a frame)"""
        n, fl = C.c_int32(0), C.c_int32(0)
        _check(self.L, self.L.orbfe_aruco_batch_status(self.h, C.byref(n), C.byref(fl)), "orbfe_aruco_batch_status")
        return n.value, fl.value

    def set_big_frames(self, on=True):
        _check(self.L, self.L.orbfe_aruco_set_big_frames(self.h, int(on)), "orbfe_aruco_set_big_frames")

    # stage read-back for parity tests
    def thresholded(self, frame=0):
        out = np.zeros(self._shape, np.uint8)
        _check(self.L, self.L.orbfe_aruco_debug_image(self.h, frame, 0, _p(out)), "debug_image")
        return out

    def pyramid_level(self, level, frame=0):
        """Debug: level >= 1 of the detector's /2 pyramid of the last batch (None past the last level)."""
        out = np.zeros(self._shape, np.uint8)
        if self.L.orbfe_aruco_debug_image(self.h, frame, level + 1, _p(out)) != 0:
            return None
        h, w = self._shape
        for _ in range(level):
            w, h = w // 2, h // 2        # exact halves only (the levels this accessor is for)
        return out.reshape(-1)[:w * h].reshape(h, w).copy()

    def counts(self, frame=0):
        out = np.zeros(4, np.int32)
        _check(self.L, self.L.orbfe_aruco_debug_image(self.h, frame, 100, _p(out)), "debug_image")
        return dict(nkept=int(out[0]), nrect=int(out[1]), flags=int(out[2]), ncand=int(out[3]) & 0x3fffffff,
                    fell_back=bool(int(out[3]) >> 30))   # the relay contour kernel handed the frame to the legacy one

    def debug_control(self, key, value):
        """orbfe_aruco_debug_control: a named test / diagnosis switch of this handle (include/orbfe.h lists the keys)."""
        _check(self.L, self.L.orbfe_aruco_debug_control(self.h, key.encode(), int(value)), "aruco_debug_control")

    def force_legacy_contours(self, on=True):
        """Debug: run every frame through the single-walker contour kernel (the relay kernel's fallback)."""
        self.debug_control("legacy_contours", on)

    def set_tiled_contours(self, mode):
        """Debug: the tiled contour path (aruco_tiles.hip) None = by frame / batch size (default), True = every batch, False = never."""
        self.debug_control("tiled_contours", -1 if mode is None else bool(mode))

    def set_speck_passes(self, on=True):
        """Debug: the speck passes between threshold and contours (k_speck_clean) on / off (default); the results do not change."""
        self.debug_control("speck_passes", on)

    def set_threshold_on_matrix_cores(self, on=True):
        """True: k_threshold_mfma wherever it applies (windows up to 15); False: k_threshold_pyr, or the generic k_adaptive_threshold
        where that is switched off or does not apply; None: the default rule -- the matrix-core kernel for calls of 8 frames and more,
        k_threshold_pyr (one launch instead of five) for the drop-in call's few."""
        self.debug_control("threshold_mfma", -1 if on is None else bool(on))

    def set_threshold_pyramid_kernel(self, on=True):
        """k_threshold_pyr (threshold + the /2 pyramid levels a tile holds, the default where it applies) / the generic
        k_adaptive_threshold + k_half_area4 (with the matrix-core kernel switched off as well; else that one takes the frame)."""
        self.debug_control("threshold_pyr", on)

    def set_half_pyramid_kernel(self, on=True):
        """k_half_pyr (the leading exact /2 levels in one launch, default) / one k_half_area4 launch a level."""
        self.debug_control("half_pyr", on)

    def set_speck_passes_in_kernel(self, on=True):
        """Debug: the speck passes inside the one-workgroup relay kernels (full batches of frames whose bit image fits LDS) on / off (default)."""
        self.debug_control("speck_passes_in_kernel", on)

    def contour_image(self, frame=0):
        """Debug: the bit image the contour kernels of the last batch read from HBM (the thresholded image after the speck passes where
        they ran as a launch; with the in-kernel passes the cleaned image only exists in LDS and this is the thresholded image)."""
        out = np.zeros(self._shape, np.uint8)
        _check(self.L, self.L.orbfe_aruco_debug_image(self.h, frame, 104, _p(out)), "debug_image")
        return out

    def contour_retries(self):
        """Debug: how many batches of this detector were done again on the next contour path (tiled -> one workgroup -> single walker)
        because a frame exceeded a capacity of the one they ran on."""
        return _check(self.L, self.L.orbfe_aruco_debug_contour_retries(self.h), "debug_contour_retries")

    def rects(self, frame=0):
        out = np.zeros(self.capacity, RECT_DTYPE)
        _check(self.L, self.L.orbfe_aruco_debug_image(self.h, frame, 101, _p(out)), "debug_image")
        return out[:self.counts(frame)["nrect"]]

    def set_aux_stream(self, stream_ptr):
        """Run the detector's forked launches (pyramid) on the caller's stream (None: the handle's own)."""
        _check(self.L, self.L.orbfe_aruco_set_aux_stream(self.h, stream_ptr), "set_aux_stream")

    def enable_kernel_timing(self, on=True):
        self.debug_control("kernel_timing", on)

    def kernel_times_us(self, median=False):
        """Stage times of the last batch, or (median=True) the per-stage median over the batches since timing was enabled."""
        out = np.zeros(32, np.float32)
        n = self.L.orbfe_aruco_debug_kernel_times(self.h, _p(out), -32 if median else 32)
        return out[:n]

    @staticmethod
    def algorithmic_bytes(rows, cols):
        """Per-frame algorithmic bytes of each ArUco stage (terms of SURVEY 8d's B_aruco ~ 3.33 W H)."""
        wh = rows * cols
        return {"aruco_threshold": wh + wh // 8, "aruco_pyramid": wh + wh // 3, "aruco_contours": wh // 8,
                "aruco_decode": 0, "aruco_finalize": 0}


# ------------------------------------------------------------------------------- LocalBundleAdjustment (local mapping) ----
LBA_MAX_FREE_POSES, LBA_MAX_OBSERVATIONS, LBA_STOPPED = _defines("LBA_MAX_FREE_POSES", "LBA_MAX_OBSERVATIONS", "LBA_STOPPED")
LBA_RESULT_DTYPE = header.dtype("orbfe_lba_result")
assert LBA_RESULT_DTYPE.itemsize == 36


def lba_arrays(pb):
    """The flat arrays of a LocalBundleAdjustment problem, contiguous and typed as include/orbfe.h takes them.  pb: a dict with Tcw
    (nkf x 3 x 4), kf_fixed, x3Dw (np x 3), obs_offset (np + 1), obs_kf, obs_xy (nobs x 2), obs_octave, K (3 x 3 or fx, fy, cx, cy),
    inv_level_sigma2, and optionally Twm (nma x 3 x 4), marker_local (nma x 4 x 3), mobs_offset (nma + 1), mobs_kf, mobs_corners
    (nmobs x 4 x 2), marker_info (25), use_markers (1 when markers are given)."""
    c = lambda k, t, shape: np.ascontiguousarray(np.asarray(pb.get(k, np.zeros(0)), t).reshape(shape))
    a = dict(Tcw=c("Tcw", np.float32, (-1, 12)).copy(), kf_fixed=c("kf_fixed", np.uint8, -1), x3Dw=c("x3Dw", np.float32, (-1, 3)).copy(),
             obs_offset=c("obs_offset", np.int32, -1), obs_kf=c("obs_kf", np.int32, -1), obs_xy=c("obs_xy", np.float32, (-1, 2)),
             obs_octave=c("obs_octave", np.int32, -1), K4=_K4(pb["K"]), inv_level_sigma2=c("inv_level_sigma2", np.float32, -1),
             Twm=c("Twm", np.float32, (-1, 12)).copy(), marker_local=c("marker_local", np.float32, (-1, 12)),
             mobs_offset=c("mobs_offset", np.int32, -1), mobs_kf=c("mobs_kf", np.int32, -1), mobs_corners=c("mobs_corners", np.float32, (-1, 8)))
    a["marker_info"] = float(pb.get("marker_info", 25.0))
    a["use_markers"] = int(pb.get("use_markers", 1 if len(a["Twm"]) else 0))
    if len(a["Tcw"]) != len(a["kf_fixed"]) or len(a["obs_kf"]) != len(a["obs_xy"]) or len(a["obs_kf"]) != len(a["obs_octave"]) or \
            len(a["obs_offset"]) != (len(a["x3Dw"]) + 1 if len(a["x3Dw"]) else len(a["obs_offset"])) or len(a["Twm"]) != len(a["marker_local"]) or \
            len(a["mobs_kf"]) != len(a["mobs_corners"]) or len(a["mobs_offset"]) != (len(a["Twm"]) + 1 if len(a["Twm"]) else len(a["mobs_offset"])):
        raise ValueError("LocalBundleAdjustment: array lengths do not agree")
    return a


def _lba_problem_args(a):
    q = _ptr_or_none
    return [q(a["Tcw"]), q(a["kf_fixed"]), len(a["Tcw"]), q(a["x3Dw"]), len(a["x3Dw"]), q(a["obs_offset"]), q(a["obs_kf"]), q(a["obs_xy"]),
            q(a["obs_octave"]), len(a["obs_kf"]), _p(a["K4"]), q(a["inv_level_sigma2"]), len(a["inv_level_sigma2"]), q(a["Twm"]),
            q(a["marker_local"]), len(a["Twm"]), q(a["mobs_offset"]), q(a["mobs_kf"]), q(a["mobs_corners"]), len(a["mobs_kf"]),
            a["marker_info"], a["use_markers"]]


def lba_scratch_bytes(nkf, np_, nobs, nma, nmobs):
    return int(load().orbfe_lba_scratch_bytes(int(nkf), int(np_), int(nobs), int(nma), int(nmobs)))


def local_bundle_adjustment(pb, stop=False, device=0):
    """Optimizer::LocalBundleAdjustment (Optimizer.cc:892-1242, behind the collect step) on the GPU, host arrays.  pb as lba_arrays
    takes it; stop = the value of *pbStopFlag at the call.  Returns dict(Tcw (nkf x 3 x 4), x3Dw, Twm, erase (a byte per observation
    slot), result (LBA_RESULT_DTYPE)); the inputs are not modified."""
    L = load()
    a = lba_arrays(pb)
    erase = np.zeros(len(a["obs_kf"]), np.uint8)
    res = np.zeros(1, LBA_RESULT_DTYPE)
    flag = np.array([1 if stop else 0], np.uint8)
    _check(L, L.orbfe_local_bundle_adjustment(*(_lba_problem_args(a) + [_p(flag), _ptr_or_none(erase), _p(res), device])),
           "orbfe_local_bundle_adjustment")
    return dict(Tcw=a["Tcw"].reshape(-1, 3, 4), x3Dw=a["x3Dw"], Twm=a["Twm"].reshape(-1, 3, 4), erase=erase, result=res[0])


def local_bundle_adjustment_device(d, nkf, np_, nobs, nma, nmobs, K, inv_level_sigma2, marker_info, use_markers, capacity=0, stream=0):
    """orbfe_local_bundle_adjustment_device: d maps the argument names of include/orbfe.h without their d_ prefix (Tcw, kf_fixed, x3Dw,
    obs_offset, obs_kf, obs_xy, obs_octave, obs_feature, kps, Twm, marker_local, mobs_offset, mobs_kf, mobs_corners, stop, erase, res,
    scratch) to device addresses (0 / missing = NULL) and scratch_bytes to a size.  Asynchronous on `stream`."""
    L = load()
    g = lambda k: d.get(k) or None
    sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    _check(L, L.orbfe_local_bundle_adjustment_device(
        g("Tcw"), g("kf_fixed"), int(nkf), g("x3Dw"), int(np_), g("obs_offset"), g("obs_kf"), g("obs_xy"), g("obs_octave"), g("obs_feature"),
        g("kps"), int(capacity), int(nobs), _p(_K4(K)), _p(sig), len(sig), g("Twm"), g("marker_local"), int(nma), g("mobs_offset"),
        g("mobs_kf"), g("mobs_corners"), int(nmobs), float(marker_info), int(use_markers), g("stop"), g("erase"), g("res"), g("scratch"),
        int(d.get("scratch_bytes", 0)), stream), "orbfe_local_bundle_adjustment_device")


def _ba_system(nv, b, Hpp, Hll, chi2, x, n):
    """what lba_inspect and gba_inspect return of one linearisation and the first trial, from the buffers the library filled (n points)"""
    v = int(nv[0])
    return dict(nv=v, b_pose=b[:6 * v].reshape(v, 6), b_point=b[6 * v:6 * v + 3 * n].reshape(n, 3), Hpp=Hpp[:v], Hll=Hll[:n], chi2=chi2[0],
                lambda0=chi2[1], x_pose=x[:6 * v].reshape(v, 6), x_point=x[6 * v:6 * v + 3 * n].reshape(n, 3))


def _front_tree(tree, nv):
    """what essential_graph_inspect and gba_inspect return of the elimination tree over nv vertices: nlevels, node_of, order_of (per
    vertex), parent, level, nown, nb (per node)"""
    nn = int(tree[0])
    nodes = tree[2 + 2 * nv:2 + 2 * nv + 4 * nn].reshape(nn, 4)
    return dict(nlevels=int(tree[1]), node_of=tree[2:2 + nv].copy(), order_of=tree[2 + nv:2 + 2 * nv].copy(), parent=nodes[:, 0].copy(),
                level=nodes[:, 1].copy(), nown=nodes[:, 2].copy(), nb=nodes[:, 3].copy())


def lba_inspect(pb, device=0):
    """orbfe_lba_inspect: one linearisation and the first trial.  Returns dict(nv, b_pose (nv x 6), b_point (np x 3), Hpp (nv x 6 x 6),
    Hll (np x 6: xx xy xz yy yz zz), chi2, lambda0, x_pose (nv x 6), x_point (np x 3))."""
    L = load()
    a = lba_arrays(pb)
    n = len(a["x3Dw"])
    nv = np.zeros(1, np.int32)
    b = np.zeros(6 * LBA_MAX_FREE_POSES + 3 * n); x = np.zeros_like(b)
    Hpp = np.zeros((LBA_MAX_FREE_POSES, 6, 6)); Hll = np.zeros((max(n, 1), 6)); chi2 = np.zeros(2)
    _check(L, L.orbfe_lba_inspect(*(_lba_problem_args(a) + [_p(nv), _p(b), _p(Hpp), _p(Hll), _p(chi2), _p(x), device])), "orbfe_lba_inspect")
    return _ba_system(nv, b, Hpp, Hll, chi2, x, n)


# ------------------------------------------------------------------------------- OptimizeEssentialGraph (loop closing) ----
EG_MAX_KEYFRAMES, EG_MAX_EDGES = _defines("EG_MAX_KEYFRAMES", "EG_MAX_EDGES")
EG_RESULT_DTYPE = header.dtype("orbfe_eg_result")
assert EG_RESULT_DTYPE.itemsize == 40


def eg_arrays(pb):
    """The flat arrays of an OptimizeEssentialGraph problem, contiguous and typed as include/orbfe.h takes them.  pb: a dict with Tcw
    (nkf x 3 x 4), fixed, edge_i, edge_j, edge_kind, and optionally kf_id, corrected_pos + corrected (nc x 8: quaternion x y z w, t, s),
    noncorrected_pos + noncorrected, x3Dw (np x 3) + point_ref, iterations (20), fix_scale (1), leaf_vertices (0)."""
    c = lambda k, t, shape: np.ascontiguousarray(np.asarray(pb.get(k, np.zeros(0)), t).reshape(shape))
    a = dict(Tcw=c("Tcw", np.float32, (-1, 12)), corrected_pos=c("corrected_pos", np.int32, -1), corrected=c("corrected", np.float64, (-1, 8)),
             noncorrected_pos=c("noncorrected_pos", np.int32, -1), noncorrected=c("noncorrected", np.float64, (-1, 8)),
             edge_i=c("edge_i", np.int32, -1), edge_j=c("edge_j", np.int32, -1), edge_kind=c("edge_kind", np.int32, -1),
             x3Dw=c("x3Dw", np.float32, (-1, 3)), point_ref=c("point_ref", np.int32, -1))
    a["kf_id"] = c("kf_id", np.int32, -1) if "kf_id" in pb else np.arange(len(a["Tcw"]), dtype=np.int32)
    a["fixed"] = int(pb["fixed"])
    a["iterations"] = int(pb.get("iterations", 20))
    a["fix_scale"] = int(pb.get("fix_scale", 1))
    a["leaf_vertices"] = int(pb.get("leaf_vertices", 0))
    if len(a["corrected_pos"]) != len(a["corrected"]) or len(a["noncorrected_pos"]) != len(a["noncorrected"]) or \
            len(a["edge_i"]) != len(a["edge_j"]) or len(a["edge_i"]) != len(a["edge_kind"]) or len(a["x3Dw"]) != len(a["point_ref"]) or \
            len(a["kf_id"]) != len(a["Tcw"]):
        raise ValueError("OptimizeEssentialGraph: array lengths do not agree")
    return a


def _eg_graph_args(a, q=None):
    q = q or _ptr_or_none
    return [_ptr_or_none(a["kf_id"]), q(a["Tcw"]), len(a["Tcw"]), a["fixed"], q(a["corrected_pos"]), q(a["corrected"]), len(a["corrected"]),
            q(a["noncorrected_pos"]), q(a["noncorrected"]), len(a["noncorrected"]), _ptr_or_none(a["edge_i"]), _ptr_or_none(a["edge_j"]),
            _ptr_or_none(a["edge_kind"]), len(a["edge_i"])]


def essential_graph_scratch_bytes(nkf, nedges, npoints, leaf_vertices=0):
    return int(load().orbfe_essential_graph_scratch_bytes(int(nkf), int(nedges), int(npoints), int(leaf_vertices)))


def optimize_essential_graph(pb, device=0):
    """Optimizer::OptimizeEssentialGraph (Optimizer.cc:1245-1542, behind the collect step) on the GPU, host arrays.  pb as eg_arrays
    takes it.  Returns dict(Tcw (nkf x 3 x 4), x3Dw, Siw (nkf x 8), result (EG_RESULT_DTYPE))."""
    L = load()
    a = eg_arrays(pb)
    nkf, n = len(a["Tcw"]), len(a["x3Dw"])
    Tout = np.zeros((nkf, 12), np.float32); Xout = np.zeros((n, 3), np.float32); Siw = np.zeros((nkf, 8)); res = np.zeros(1, EG_RESULT_DTYPE)
    _check(L, L.orbfe_optimize_essential_graph(*(_eg_graph_args(a) + [_ptr_or_none(a["x3Dw"]), _ptr_or_none(a["point_ref"]), n, a["iterations"],
                                                                      a["fix_scale"], a["leaf_vertices"], _p(Tout), _ptr_or_none(Xout), _p(Siw),
                                                                      _p(res), device])), "orbfe_optimize_essential_graph")
    return dict(Tcw=Tout.reshape(-1, 3, 4), x3Dw=Xout, Siw=Siw, result=res[0])


def optimize_essential_graph_device(pb, d, stream=0):
    """orbfe_optimize_essential_graph_device: pb as eg_arrays takes it, of which the graph (kf_id, edge_i, edge_j, edge_kind) and the
    sizes are read; d maps the d_ argument names of include/orbfe.h without their prefix (Tcw, corrected_pos, corrected,
    noncorrected_pos, noncorrected, x3Dw, point_ref, Tcw_out, x3Dw_out, Siw_out, res, scratch) to device addresses (0 / missing = NULL)
    and scratch_bytes to a size.  Asynchronous on `stream`."""
    L = load()
    a = eg_arrays(pb)
    g = lambda k: d.get(k) or None
    _check(L, L.orbfe_optimize_essential_graph_device(
        _ptr_or_none(a["kf_id"]), g("Tcw"), len(a["Tcw"]), a["fixed"], g("corrected_pos"), g("corrected"), len(a["corrected"]), g("noncorrected_pos"),
        g("noncorrected"), len(a["noncorrected"]), _ptr_or_none(a["edge_i"]), _ptr_or_none(a["edge_j"]), _ptr_or_none(a["edge_kind"]), len(a["edge_i"]),
        g("x3Dw"), g("point_ref"), len(a["x3Dw"]), a["iterations"], a["fix_scale"], a["leaf_vertices"], g("Tcw_out"), g("x3Dw_out"), g("Siw_out"),
        g("res"), g("scratch"), int(d.get("scratch_bytes", 0)), stream), "orbfe_optimize_essential_graph_device")


def essential_graph_inspect(pb, device=0):
    """orbfe_essential_graph_inspect: one linearisation and one solve at lambda0.  Returns dict(err (ne x 7), Ji, Jj (ne x 7 x 7), Hd
    (nkf x 7 x 7), b (nkf x 7), chi2, lambda0, solved, x (nkf x 7), nlevels, node_of, order_of (nkf), parent, level, nown, nb (per node))."""
    L = load()
    a = eg_arrays(pb)
    nkf, ne = len(a["Tcw"]), len(a["edge_i"])
    err = np.zeros((ne, 7)); Ji = np.zeros((ne, 7, 7)); Jj = np.zeros((ne, 7, 7)); Hd = np.zeros((nkf, 7, 7)); b = np.zeros((nkf, 7))
    chi2 = np.zeros(3); x = np.zeros((nkf, 7)); tree = np.zeros(10 * nkf + 10, np.int32)
    _check(L, L.orbfe_essential_graph_inspect(*(_eg_graph_args(a) + [a["fix_scale"], a["leaf_vertices"], _p(err), _p(Ji), _p(Jj), _p(Hd), _p(b),
                                                                     _p(chi2), _p(x), _p(tree), device])), "orbfe_essential_graph_inspect")
    return dict(err=err, Ji=Ji, Jj=Jj, Hd=Hd, b=b, chi2=chi2[0], lambda0=chi2[1], solved=bool(chi2[2]), x=x, **_front_tree(tree, nkf))


# ------------------------------------------------------------------------------- GlobalBundleAdjustment (map-wide BA) ----
GBA_MAX_POSES, GBA_MAX_OBSERVATIONS, GBA_STOPPED = _defines("GBA_MAX_POSES", "GBA_MAX_OBSERVATIONS", "GBA_STOPPED")
GBA_RESULT_DTYPE = header.dtype("orbfe_gba_result")
assert GBA_RESULT_DTYPE.itemsize == 48


def gba_arrays(pb):
    """The flat arrays of a GlobalBundleAdjustment problem: lba_arrays(pb) plus the options iterations (10), robust (0) and
    leaf_vertices (0)."""
    a = lba_arrays(pb)
    a["iterations"] = int(pb.get("iterations", 10))
    a["robust"] = int(pb.get("robust", 0))
    a["leaf_vertices"] = int(pb.get("leaf_vertices", 0))
    return a


def gba_scratch_bytes(nkf, np_, nobs, nma, nmobs, leaf_vertices=0):
    return int(load().orbfe_gba_scratch_bytes(int(nkf), int(np_), int(nobs), int(nma), int(nmobs), int(leaf_vertices)))


def global_bundle_adjustment(pb, stop=False, device=0):
    """Optimizer::BundleAdjustment (Optimizer.cc:49-307, behind the collect step) on the GPU, host arrays.  pb as gba_arrays takes it;
    stop = the value of *pbStopFlag at the call.  Returns dict(Tcw (nkf x 3 x 4), x3Dw, Twm, result (GBA_RESULT_DTYPE)); the inputs
    are not modified."""
    L = load()
    a = gba_arrays(pb)
    res = np.zeros(1, GBA_RESULT_DTYPE)
    flag = np.array([1 if stop else 0], np.uint8)
    _check(L, L.orbfe_global_bundle_adjustment(*(_lba_problem_args(a) + [a["iterations"], a["robust"], _p(flag), a["leaf_vertices"], _p(res), device])),
           "orbfe_global_bundle_adjustment")
    return dict(Tcw=a["Tcw"].reshape(-1, 3, 4), x3Dw=a["x3Dw"], Twm=a["Twm"].reshape(-1, 3, 4), result=res[0])


def global_bundle_adjustment_device(pb, d, capacity=0, stream=0):
    """orbfe_global_bundle_adjustment_device: pb as gba_arrays takes it, of which the graph (kf_fixed, obs_offset, obs_kf, mobs_offset,
    mobs_kf), the camera, the options and the sizes are read; d maps the d_ argument names of include/orbfe.h without their prefix
    (Tcw, x3Dw, obs_xy, obs_octave, obs_feature, kps, Twm, marker_local, mobs_corners, stop, res, scratch) to device addresses
    (0 / missing = NULL) and scratch_bytes to a size.  Asynchronous on `stream`."""
    L = load()
    a = gba_arrays(pb)
    g = lambda k: d.get(k) or None
    q = _ptr_or_none
    _check(L, L.orbfe_global_bundle_adjustment_device(
        g("Tcw"), q(a["kf_fixed"]), len(a["Tcw"]), g("x3Dw"), len(a["x3Dw"]), q(a["obs_offset"]), q(a["obs_kf"]), g("obs_xy"), g("obs_octave"),
        g("obs_feature"), g("kps"), int(capacity), len(a["obs_kf"]), _p(a["K4"]), q(a["inv_level_sigma2"]), len(a["inv_level_sigma2"]), g("Twm"),
        g("marker_local"), len(a["Twm"]), q(a["mobs_offset"]), q(a["mobs_kf"]), g("mobs_corners"), len(a["mobs_kf"]), a["marker_info"], a["use_markers"],
        a["iterations"], a["robust"], g("stop"), a["leaf_vertices"], g("res"), g("scratch"), int(d.get("scratch_bytes", 0)), stream),
        "orbfe_global_bundle_adjustment_device")


def gba_inspect(pb, device=0):
    """orbfe_gba_inspect: one linearisation and the first trial.  Returns dict(nv, b_pose (nv x 6), b_point (np x 3), Hpp (nv x 6 x 6),
    Hll (np x 6: xx xy xz yy yz zz), chi2, lambda0, solved, x_pose (nv x 6), x_point (np x 3), nlevels, node_of, order_of (nv), parent,
    level, nown, nb (per node))."""
    L = load()
    a = gba_arrays(pb)
    n, V = len(a["x3Dw"]), len(a["Tcw"]) + len(a["Twm"])
    nv = np.zeros(1, np.int32)
    b = np.zeros(6 * V + 3 * n + 1); x = np.zeros_like(b)
    Hpp = np.zeros((max(V, 1), 6, 6)); Hll = np.zeros((max(n, 1), 6)); chi2 = np.zeros(3); tree = np.zeros(10 * V + 10, np.int32)
    _check(L, L.orbfe_gba_inspect(*(_lba_problem_args(a) + [a["robust"], a["leaf_vertices"], _p(nv), _p(b), _p(Hpp), _p(Hll), _p(chi2), _p(x), _p(tree),
                                                          device])), "orbfe_gba_inspect")
    return dict(_ba_system(nv, b, Hpp, Hll, chi2, x, n), solved=bool(chi2[2]), **_front_tree(tree, int(nv[0])))
