"""Seeded synthetic keyframes for the CreateNewMapPoints tests, the sequential CPU reference (tests/new_points_ref.cpp with the oracle's
SearchForTriangulation between the triangulations) and the float64 second opinion.

A scene is one current keyframe and its neighbours looking at one cloud of landmarks.  Every keyframe sees every landmark, in an
order of its own; a share of the landmarks is mapped already (valid, x3Dw = the true point), the rest is free.  Descriptors are one
random 256-bit string per landmark with a few bits flipped per keyframe, so that only true correspondences are closer than TH_LOW;
the FeatureVector groups features by landmark id modulo NODES (no vocabulary is needed for that).  Pixel noise is Gaussian; a share
of the free features of a neighbour is moved by tens of pixels (gross outliers)."""
import ctypes as C
import functools

import numpy as np

import ref_build
from initializer_cases import KP_DTYPE, rot

K4 = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
NLEVELS = 8
SCALE = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)
RATIO = float(np.float32(1.5) * SCALE[1])
NODES = 37
PAIR_DTYPE = np.dtype([("baseline", np.float32), ("median_depth", np.float32), ("n_depths", np.int32), ("skipped", np.int32)])
RESULT_DTYPE = np.dtype([("n_matches", np.int32), ("n_new", np.int32), ("status", np.int32)])
FLT_EPS = float(np.finfo(np.float32).eps)
COS_GATE, COS_BAND, REL_BAND, CHI2 = 0.9998, 1e-6, 1e-4, 5.991


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def ref():
    L = ref_build.build_shared("new_points_ref.cpp")
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.nmp_ref_prepare.restype = None
    L.nmp_ref_prepare.argtypes = [i32] + [vp] * 9
    L.nmp_ref_triangulate.restype = i32
    L.nmp_ref_triangulate.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, f32] + [vp] * 6
    return L


def tcw(R, t):
    return np.ascontiguousarray(np.c_[np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], np.float32)


def project(T, X):
    Xc = X @ T[:, :3].astype(np.float64).T + T[:, 3].astype(np.float64)
    return Xc[:, :2] / Xc[:, 2:3] * K4[:2].astype(np.float64) + K4[2:].astype(np.float64), Xc[:, 2]


def keypoints(uv, octave):
    k = np.zeros(len(uv), KP_DTYPE)
    k["x"], k["y"] = uv[:, 0], uv[:, 1]
    k["size"] = 31; k["angle"] = 0; k["response"] = 1e-3; k["octave"] = octave; k["class_id"] = -1
    return k


def feature_vector(landmark):
    """(node, offset, feature) of a keyframe whose feature i shows landmark[i]: nodes ascending, features ascending inside a node"""
    node = np.asarray(landmark) % NODES
    ids = np.unique(node)
    feats = [np.flatnonzero(node == i) for i in ids]
    off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    return ids.astype(np.uint32), off, (np.concatenate(feats) if feats else np.zeros(0)).astype(np.uint32)


def scene(seed, n, neighbours=1, noise=0.7, outliers=0.2, baseline=(0.05, 0.4), depth=(1.5, 9.0), mapped=0.4, shared=True, n_of=None):
    """-> dict(frames=[cur, nb1, ...], X (landmarks), landmark=[per frame: landmark id of feature i]).  A frame is a dict with kps, desc,
    fv, x3Dw, valid, Tcw.  n_of: features per frame (default n everywhere; a frame with fewer sees the first landmarks only).
    shared=True gives every neighbour the same free landmarks, so that later neighbours compete for the current keyframe's features."""
    rng = np.random.default_rng(seed)
    nf = neighbours + 1
    n_of = [n] * nf if n_of is None else list(n_of)
    N = max(max(n_of), 1)
    uv = np.stack([rng.uniform(60, 580, N), rng.uniform(60, 420, N)], 1)
    z = rng.uniform(depth[0], depth[1], N)
    X = np.c_[(uv - K4[2:]) / K4[:2], np.ones(N)] * z[:, None]
    is_mapped = rng.random(N) < mapped
    octave = rng.integers(0, 4, N)
    ldesc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    frames, landmark = [], []
    for f in range(nf):
        if f == 0:
            R, t = np.eye(3), np.zeros(3)
        else:
            R = rot(rng.normal(size=3), rng.uniform(0.5, 4.0))
            d = rng.normal(size=3); d[2] *= 0.3
            c = d / np.linalg.norm(d) * rng.uniform(*baseline)
            t = -R @ c
        T = tcw(R, t)
        m = n_of[f]
        order = rng.permutation(N)[:m] if m == N else rng.permutation(m)
        p, _ = project(T, X[order])
        p = p + rng.normal(size=p.shape) * noise
        if f > 0 and outliers > 0:
            bad = (rng.random(m) < outliers) & ~is_mapped[order]
            p[bad] += rng.uniform(-40, 40, (int(bad.sum()), 2))
        oc = np.clip(octave[order] + (rng.integers(-1, 2, m) if f > 0 else 0), 0, NLEVELS - 1)
        desc = ldesc[order].copy()
        flip = rng.integers(0, 256, (m, 6))
        for j in range(flip.shape[1]):
            desc[np.arange(m), flip[:, j] // 8] ^= (1 << (flip[:, j] % 8)).astype(np.uint8)
        valid = is_mapped[order].astype(np.uint8)
        if f > 0 and not shared:
            valid |= (rng.random(m) < 0.3).astype(np.uint8)
        x3Dw = np.where(valid[:, None] != 0, X[order], 0).astype(np.float32)
        frames.append(dict(kps=keypoints(p.astype(np.float32), oc), desc=desc, fv=feature_vector(order), x3Dw=x3Dw, valid=valid, Tcw=T))
        landmark.append(order)
    return dict(frames=frames, X=X, landmark=landmark)


def true_matches(sc, f2, rng=None, wrong=0.0):
    """match12 of the current keyframe against frame f2 over the free features of both: the true correspondences, a share replaced
    by a random other free feature (kept unique on side 2)"""
    l1, l2 = sc["landmark"][0], sc["landmark"][f2]
    where2 = {int(l): i for i, l in enumerate(l2)}
    v1, v2 = sc["frames"][0]["valid"], sc["frames"][f2]["valid"]
    m12 = np.full(len(l1), -1, np.int32)
    for i, l in enumerate(l1):
        j = where2.get(int(l), -1)
        if j >= 0 and not v1[i] and not v2[j]:
            m12[i] = j
    if rng is not None and wrong > 0:
        idx = np.flatnonzero(m12 >= 0)
        pick = idx[rng.random(len(idx)) < wrong]
        if len(pick) > 1:
            m12[pick] = m12[np.roll(pick, 1)]
    return m12


# ------------------------------------------------------------------------------------------------- the CPU reference
def ref_prepare(cur, nb):
    F = np.zeros(9, np.float32); e = np.zeros(2, np.float32); rf = np.zeros(2, np.float32); ri = np.zeros(2, np.int32)
    x = np.ascontiguousarray(nb["x3Dw"], np.float32); v = np.ascontiguousarray(nb["valid"], np.uint8)
    ref().nmp_ref_prepare(len(v), _p(x), _p(v), _p(cur["Tcw"]), _p(nb["Tcw"]), _p(K4), _p(F), _p(e), _p(rf), _p(ri))
    rec = np.zeros(1, PAIR_DTYPE)
    rec["baseline"], rec["median_depth"], rec["n_depths"], rec["skipped"] = rf[0], rf[1], ri[0], ri[1]
    return F, e, rec[0]


def ref_triangulate(k1, T1, k2, T2, m12, state=None, scale=SCALE, sigma2=SIGMA2, ratio=RATIO):
    """one pair's match list.  state = (x3Dw1, valid1, x3Dw2, valid2), updated in place, or None.  -> dict like binding.new_points_inspect"""
    n1 = len(k1)
    status = np.zeros(n1, np.uint8); x3D = np.zeros((n1, 3), np.float32); normal = np.zeros((n1, 3), np.float32)
    dist = np.zeros((n1, 2), np.float32); q = np.zeros((n1, 6), np.float32); res = np.zeros(3, np.int32)
    k1 = np.ascontiguousarray(k1, KP_DTYPE); k2 = np.ascontiguousarray(k2, KP_DTYPE); m12 = np.ascontiguousarray(m12, np.int32)
    s = [None] * 4 if state is None else list(state)
    rc = ref().nmp_ref_triangulate(_p(k1), n1, _p(s[0]), _p(s[1]), _p(np.ascontiguousarray(T1, np.float32)), _p(k2), len(k2), _p(s[2]), _p(s[3]),
                                   _p(np.ascontiguousarray(T2, np.float32)), _p(m12), _p(K4), _p(np.ascontiguousarray(scale, np.float32)),
                                   _p(np.ascontiguousarray(sigma2, np.float32)), len(scale), np.float32(ratio), _p(status), _p(x3D), _p(normal),
                                   _p(dist), _p(q), _p(res))
    r = np.zeros(1, RESULT_DTYPE)
    r["n_matches"], r["n_new"], r["status"] = res
    return dict(rc=rc, status=status, x3D=x3D, normal=normal, dist=dist, quantities=q, result=r[0])


def ref_sequence(frames, pairs=None, ordered=True, check_orientation=False):
    """CreateNewMapPoints over a pair list (default: frames[0] against frames[1:]), pair after pair (ordered) or every pair's search on
    the state at entry (the single-launch semantics).  prepare always sees the state at entry, as the device chain's one launch does.
    -> (per pair: dict with F12, epipole, prep, match12, nmatches + ref_triangulate's; the final per-frame (x3Dw, valid) list)"""
    import oracle_lib
    pairs = [(0, p) for p in range(1, len(frames))] if pairs is None else pairs
    st = [(np.array(f["x3Dw"], np.float32), np.array(f["valid"], np.uint8)) for f in frames]
    entry = [(x.copy(), v.copy()) for x, v in st]
    out = []
    for a, b in pairs:
        cur, nb = frames[a], frames[b]
        F, e, rec = ref_prepare(dict(cur, x3Dw=entry[a][0], valid=entry[a][1]), dict(nb, x3Dw=entry[b][0], valid=entry[b][1]))
        src = st if ordered else entry
        nm, m12 = oracle_lib.search_for_triangulation(cur["kps"], cur["desc"], cur["fv"], nb["kps"], nb["desc"], nb["fv"], F.reshape(3, 3), e, SCALE,
                                                      SIGMA2, src[a][1], src[b][1], check_orientation)
        r = ref_triangulate(cur["kps"], cur["Tcw"], nb["kps"], nb["Tcw"], m12, (st[a][0], st[a][1], st[b][0], st[b][1]))
        r.update(F12=F, epipole=e, prep=rec, match12=m12, nmatches=nm)
        out.append(r)
    return out, st


# ------------------------------------------------------------------------------------------------- bands and second opinion
def banded(r, k1, k2, m12, scale=SCALE, sigma2=SIGMA2, ratio=RATIO):
    """boolean per side-1 feature: a gate quantity of the restatement r lies inside a band of the parity contract"""
    q, st = r["quantities"].astype(np.float64), r["status"]
    n1 = len(st)
    out = np.zeros(n1, bool)
    has = st != 0
    if not has.any():
        return out
    out |= has & (np.abs(q[:, 0] - COS_GATE) <= COS_BAND)
    j = np.where(has, m12, 0)
    th1 = CHI2 * sigma2[np.clip(k1["octave"], 0, len(sigma2) - 1)].astype(np.float64)
    th2 = CHI2 * sigma2[np.clip(k2["octave"][j], 0, len(sigma2) - 1)].astype(np.float64)
    reached1 = has & (st >= 7) | (st == 1)
    out |= reached1 & (np.abs(q[:, 1] - th1) <= REL_BAND * th1)
    reached2 = has & (st >= 8) | (st == 1)
    out |= reached2 & (np.abs(q[:, 2] - th2) <= REL_BAND * th2)
    reached3 = (st == 10) | (st == 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = np.where(q[:, 3] > 0, q[:, 4] / q[:, 3], 0.0)
    lo, hi = q[:, 5] / ratio, q[:, 5] * ratio
    out |= reached3 & ((np.abs(rd - lo) <= REL_BAND * lo) | (np.abs(rd - hi) <= REL_BAND * hi))
    return out


def dlt64(k1, T1, k2, T2, i1, i2):
    """float64 second opinion for one match: (null vector as a Euclidean point, s1, s3) of the DLT system built in float64 from the
    float32 inputs"""
    K = K4.astype(np.float64)
    a = (np.array([k1["x"][i1], k1["y"][i1]], np.float64) - K[2:]) / K[:2]
    b = (np.array([k2["x"][i2], k2["y"][i2]], np.float64) - K[2:]) / K[:2]
    A = np.stack([a[0] * T1[2] - T1[0], a[1] * T1[2] - T1[1], b[0] * T2[2] - T2[0], b[1] * T2[2] - T2[1]]).astype(np.float64)
    _, s, vt = np.linalg.svd(A)
    return vt[3, :3] / vt[3, 3], s[0], s[2]


# ------------------------------------------------------------------------------------------------- the hand-built case
def every_code_case():
    """Frames 0 .. 4 and pairs that between them give every status code 0 .. 10 at least once.
    Pair (0, 1), two proper cameras (the neighbour 0.3 m to the side and 0.5 m ahead): 0 no match; 1 a true point; 2 a point 10 km
    away; 5 the images of a point behind both cameras; 6 a point in front of the current camera and behind the neighbour; 7 / 8 a
    6 px displacement across the epipolar line at octaves (0, 0) / (7, 0); 10 a true point seen at octaves 7 and 0.
    Codes 3, 4 and 9 cannot come from two rigid poses (a null vector with w = 0 means parallel rays, which the parallax gate takes
    first; a point at the camera centre has z = 0, which the cheirality gate takes first), so they use poses a caller could only
    pass by mistake, and pin what happens then:
    pair (0, 2): frame 2 has a sheared `rotation` (row 2 = 0.5, 0, 1); both features at the principal point make column 2 of the
        DLT system exactly zero: the null vector is (0, 0, 1, 0), w == 0 -> 3, while the rays R' xn differ -> the gate passes;
    pair (4, 1): frame 4 is frame 0 with a NaN translation: the rays (R only) pass the gate, the DLT system is NaN -> 4;
    pair (0, 3): frame 3 has rows (0, 0, -1), (0, 0, 0), (0.5, 0, 1) and t = (2, 0, 0): its `centre` -R't is (0, 0, 2), the system of
        the two principal points has the null vector (0, 0, 2, 1), which one 3-4-5 Jacobi rotation gives exactly in float, both
        depths are positive and both reprojection errors 0 -> dist2 == 0 -> 9."""
    T0 = tcw(np.eye(3), np.zeros(3))
    R1 = rot(np.array([0.0, 1.0, 0.0]), 2.0)
    T1 = tcw(R1, -R1 @ np.array([0.3, 0.0, 0.5]))
    T2 = tcw(np.array([[1, 0, 0], [0, 1, 0], [0.5, 0, 1.0]]), np.array([-0.2, 0, 0]))
    T3 = tcw(np.array([[0, 0, -1.0], [0, 0, 0], [0.5, 0, 1.0]]), np.array([2.0, 0, 0]))
    T4 = T0.copy(); T4[0, 3] = np.nan
    pp = K4[2:].astype(np.float64)
    pts = np.array([[0.4, -0.2, 5.0],      # 1
                    [300.0, 100.0, 1e4],   # 2
                    [0.5, 0.3, -3.0],      # 5
                    [0.2, 0.05, 0.25],     # 6
                    [-0.6, 0.4, 4.0],      # 7
                    [0.7, 0.5, 6.0],       # 8
                    [-0.3, -0.5, 5.5]])    # 10
    uv0, _ = project(T0, pts); uv1, _ = project(T1, pts)
    # the epipolar line in frame 1 runs roughly along x + z motion: move across it (y) for 7 / 8
    uv1[4, 1] += 6.0; uv1[5, 1] += 6.0
    oc0 = np.array([0, 0, 0, 0, 0, 7, 7]); oc1 = np.array([0, 0, 0, 0, 0, 0, 0])
    n = 10
    k0 = keypoints(np.r_[uv0, [pp, pp, [100.0, 100.0]]].astype(np.float32), np.r_[oc0, [0, 0, 0]])       # 7, 8: the principal point; 9: no match
    k1 = keypoints(np.r_[uv1, np.tile([50.0, 60.0], (3, 1))].astype(np.float32), np.r_[oc1, [0, 0, 0]])
    kpp = keypoints(np.tile(pp, (n, 1)).astype(np.float32), np.zeros(n, np.int64))
    frames_k = [k0, k1, kpp, kpp, k0]
    frames_T = [T0, T1, T2, T3, T4]
    m01 = np.array([0, 1, 2, 3, 4, 5, 6, -1, -1, -1], np.int32)
    m02 = np.full(n, -1, np.int32); m02[7] = 0
    m41 = np.full(n, -1, np.int32); m41[0] = 0
    m03 = np.full(n, -1, np.int32); m03[8] = 3
    return dict(kps=frames_k, Tcw=frames_T, pairs=[(0, 1), (0, 2), (4, 1), (0, 3)], match12=[m01, m02, m41, m03], n=n)


# ------------------------------------------------------------------------------------------------- the cases the parity tests share
# name -> (seed, noise px, gross outliers, baseline range m, share of wrong matches, mapped share)
PARITY_CASES = {
    "mixed": (1, 0.7, 0.2, (0.05, 0.4), 0.1, 0.3),
    "short-baseline": (2, 0.7, 0.2, (0.05, 0.12), 0.1, 0.3),
    "noise-free": (3, 0.0, 0.0, (0.1, 0.4), 0.0, 0.0),
    "long-baseline": (4, 0.7, 0.2, (0.3, 0.4), 0.1, 0.3),
    "noise-free-at-the-gate": (5, 0.0, 0.0, (0.05, 0.1), 0.0, 0.0),
}
CAPACITY = 512
EDGE_COUNTS = (0, 1, 63, 64, 65, 257, 512)


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """-> (scene, match12 of frame 0 against frame 1, the restatement's result for it); shared, not to be modified"""
    seed, noise, out, bl, wrong, mapped = PARITY_CASES[name]
    sc = scene(seed, CAPACITY, 1, noise=noise, outliers=out, baseline=bl, mapped=mapped)
    m12 = true_matches(sc, 1, np.random.default_rng(seed), wrong)
    f0, f1 = sc["frames"]
    return sc, m12, ref_triangulate(f0["kps"], f0["Tcw"], f1["kps"], f1["Tcw"], m12)


@functools.lru_cache(maxsize=None)
def edge_case(count):
    """the all-free scene with only the first `count` of its 512 matches kept"""
    sc = scene(11, CAPACITY, 1, mapped=0.0, outliers=0.1)
    m12 = true_matches(sc, 1)
    keep = np.flatnonzero(m12 >= 0)[count:]
    m12[keep] = -1
    assert (m12 >= 0).sum() == count
    f0, f1 = sc["frames"]
    return sc, m12, ref_triangulate(f0["kps"], f0["Tcw"], f1["kps"], f1["Tcw"], m12)


def compare_pair(got, want, k1, k2, m12, label=""):
    """The parity contract for one pair: got / want are dicts with status, x3D, normal, dist, result (want also quantities).  Status
    bytes equal except inside a band (at most 5 % of the matches, printed); created points within 1e-4 relative; counts exact when
    nothing is inside a band.  Returns the number of excluded matches."""
    n1 = len(want["status"])
    gs, ws = np.asarray(got["status"])[:n1], want["status"]
    band = banded(want, k1, k2, m12)
    differ = gs != ws
    assert not np.any(differ & ~band), (label, np.flatnonzero(differ & ~band)[:8], gs[differ & ~band][:8], ws[differ & ~band][:8])
    nmatch = int((ws != 0).sum())
    excluded = int(band.sum())
    print("%s: %d of %d matches inside a band, %d status bytes differ" % (label, excluded, nmatch, int(differ.sum())))
    assert excluded <= 0.05 * nmatch, (label, excluded, nmatch)
    both = (gs == 1) & (ws == 1)
    for key in ("x3D", "normal", "dist"):
        g, w = np.asarray(got[key])[:n1][both].astype(np.float64), want[key][both].astype(np.float64)
        scale = np.linalg.norm(w, axis=1, keepdims=True)
        assert np.all(np.abs(g - w) <= 1e-4 * scale), (label, key, float(np.max(np.abs(g - w) / scale)))
    assert int(got["result"]["status"]) == int(want["result"]["status"]) == 0, label
    if excluded == 0:
        assert int(got["result"]["n_matches"]) == int(want["result"]["n_matches"]) and int(got["result"]["n_new"]) == int(want["result"]["n_new"]), label
    return excluded


def pack_frames(frames, cap, poison=True):
    """per-frame blocks of `cap` entries, poison behind every frame's valid rows: dict of arrays [F, cap, ...]"""
    F = len(frames)
    kps = np.zeros((F, cap), KP_DTYPE)
    if poison:
        kps.view(np.uint8)[...] = 0xEE          # x, y NaN-like garbage, octave 0xEEEEEEEE: must never be read
    desc = np.full((F, cap, 32), 0xAB if poison else 0, np.uint8)
    x3Dw = np.full((F, cap, 3), np.nan if poison else 0, np.float32)
    valid = np.full((F, cap), 0x5A if poison else 0, np.uint8); free = np.full((F, cap), 0xA5 if poison else 0, np.uint8)
    fn = np.zeros((F, cap), np.uint32); fo = np.zeros((F, cap + 1), np.int32); ff = np.zeros((F, cap), np.uint32)
    n = np.zeros(F, np.int32); nfv = np.zeros(F, np.int32); T = np.zeros((F, 12), np.float32)
    for f, fr in enumerate(frames):
        m = min(len(fr["kps"]), cap)
        n[f] = len(fr["kps"])
        kps[f, :m] = fr["kps"][:m]; T[f] = np.asarray(fr["Tcw"], np.float32).reshape(12)
        if "valid" in fr:
            x3Dw[f, :m] = fr["x3Dw"][:m]; valid[f, :m] = fr["valid"][:m]; free[f, :m] = fr["valid"][:m] == 0
        if "desc" in fr:
            desc[f, :m] = fr["desc"][:m]
            a, b, c = fr["fv"]
            nfv[f] = len(a); fn[f, :len(a)] = a; fo[f, :len(b)] = b; ff[f, :len(c)] = c
    return dict(kps=kps, desc=desc, x3Dw=x3Dw, valid=valid, free=free, fn=fn, fo=fo, ff=ff, n=n, nfv=nfv, Tcw=T)


@functools.lru_cache(maxsize=None)
def chain_scene():
    """one current keyframe and three neighbours that share their free landmarks; shared, not to be modified"""
    return scene(21, CAPACITY, 3, baseline=(0.15, 0.4), mapped=0.3, outliers=0.1)


@functools.lru_cache(maxsize=None)
def smoke_scene(n=200):
    """a noise-free pair with map points on both sides (the neighbour needs them for its median depth) and 20 - 40 cm of baseline"""
    return scene(31, n, 1, noise=0.0, outliers=0.0, baseline=(0.2, 0.4), mapped=0.3)
