"""Seeded synthetic loop-closure scenes for the Sim3Solver tests: one 3-D cloud seen by two keyframes whose maps differ by a known
similarity.  Camera 1 sees the points at Xc1; camera 2, moved by (R21, t21), sees them at R21 Xc1 + t21, but its map has drifted in
scale by s, so its map holds Xc2 = (R21 Xc1 + t21) / s:  Xc1 = s12 R12 Xc2 + t12 with s12 = s, R12 = R21', t12 = -R21' t21 -- what the
solver has to find.  Each map stores its points in a world frame of its own (Tcw1, Tcw2 arbitrary).  Pixel-level noise: every map
point is moved sideways by `noise` pixels' worth at its depth, independently in the two maps.  Outliers: a share of the
correspondences gets an unrelated point in map 2.  Octaves are spread over 8 levels (scale factor 1.2)."""
import numpy as np

from initializer_cases import KP_DTYPE, rot

K4 = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
COLS, ROWS = 640, 480
LEVEL_SIGMA2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2
RANSAC = (0.99, 20, 300)     # LoopClosing.cc:529

# (N, s, outlier share, fix_scale): N in {3, 19, 20, 40, 100, 1000}, s in {1, 1.3, 0.7}, outliers in {0, 0.3, 0.6}
CASES = [(3, 1.0, 0.0, True), (3, 1.3, 0.0, False), (19, 1.3, 0.0, False), (20, 0.7, 0.0, False), (40, 1.0, 0.3, True),
         (40, 1.3, 0.3, False), (100, 1.0, 0.0, True), (100, 1.3, 0.0, False), (100, 0.7, 0.3, False), (100, 1.0, 0.6, True),
         (1000, 1.3, 0.0, False), (1000, 0.7, 0.3, False), (1000, 1.0, 0.3, True), (1000, 1.3, 0.6, False)]


def case_id(c):
    return "N%d-s%g-out%g-%s" % (c[0], c[1], c[2], "fix" if c[3] else "free")


def ransac_of(c):
    """(probability, min_inliers, max_iterations) of a case: the loop closer's, except at N = 3 where min_inliers = 3 lets the
    single iteration of `N == min_inliers` run."""
    return (0.99, 3, 300) if c[0] == 3 else RANSAC


def _pose(rng, deg, tmax):
    ax = rng.normal(size=3)
    R = rot(ax, deg)
    t = rng.uniform(-tmax, tmax, 3)
    return R, t


def _kps(uv, rng):
    k = np.zeros(len(uv), KP_DTYPE)
    k["x"], k["y"] = uv[:, 0], uv[:, 1]
    k["size"] = 31; k["angle"] = rng.uniform(0, 360, len(uv)); k["response"] = rng.uniform(0, 1e-3, len(uv))
    k["octave"] = rng.integers(0, 8, len(uv)); k["class_id"] = -1
    return k


def _cloud(rng, n):
    uv = np.stack([rng.uniform(40, COLS - 40, n), rng.uniform(40, ROWS - 40, n)], 1)
    z = rng.uniform(3.0, 9.0, n)
    return np.c_[(uv - K4[2:]) / K4[:2], np.ones(n)] * z[:, None]


def _image(X):
    return X[:, :2] / X[:, 2:3] * K4[:2] + K4[2:]


def scene(N, s=1.0, outliers=0.0, fix_scale=False, seed=0, noise=1.0, angle=None, extra=12, dropped=5):
    """N kept correspondences among n1 = N + extra + dropped features of keyframe 1: `extra` without a match, `dropped` with a match
    but an invalid map point on one side (the constructor skips them).  Returns the flat inputs of orbfe_sim3_solve plus the truth
    (s12, R12, t12) and `good`: the kept correspondences (by index in keyframe 1) that are no outliers."""
    rng = np.random.default_rng(1000 * seed + N)
    angle = rng.uniform(5, 30) if angle is None else angle
    R21, t21 = _pose(rng, angle, 0.8)
    n1 = n2 = N + extra + dropped
    nm = N + dropped
    Xc1 = _cloud(rng, nm)
    Xc2 = (Xc1 @ R21.T + t21) / s
    # noise: `noise` pixels sideways at the point's depth, each map on its own
    Xc1n = Xc1 + np.c_[rng.normal(0, noise, (nm, 2)) * Xc1[:, 2:3] / K4[0], np.zeros(nm)]
    Xc2n = Xc2 + np.c_[rng.normal(0, noise, (nm, 2)) * Xc2[:, 2:3] / K4[0], np.zeros(nm)]
    nout = int(round(outliers * N))
    bad = rng.choice(N, nout, replace=False)
    Xc2n[bad] = _cloud(rng, nout) / s
    pos1 = rng.permutation(n1)[:nm]; pos2 = rng.permutation(n2)[:nm]
    all1 = _cloud(rng, n1); all2 = _cloud(rng, n2) / s
    all1[pos1] = Xc1n; all2[pos2] = Xc2n
    m12 = np.full(n1, -1, np.int32); m12[pos1] = pos2
    valid1 = np.ones(n1, np.uint8); valid2 = np.ones(n2, np.uint8)
    valid1[pos1[N:N + dropped // 2]] = 0
    valid2[pos2[N + dropped // 2:]] = 0
    # each map's world frame
    Rw1, tw1 = _pose(rng, rng.uniform(0, 180), 3.0)
    Rw2, tw2 = _pose(rng, rng.uniform(0, 180), 3.0)
    x3Dw1 = (all1 - tw1) @ Rw1          # Rcw1' (Xc - tcw1)
    x3Dw2 = (all2 - tw2) @ Rw2
    good = np.zeros(n1, bool); good[pos1[:N]] = True; good[pos1[bad]] = False
    return dict(kps1=_kps(_image(all1), rng), kps2=_kps(_image(all2), rng), x3Dw1=x3Dw1.astype(np.float32), x3Dw2=x3Dw2.astype(np.float32),
                valid1=valid1, valid2=valid2, Tcw1=np.c_[Rw1, tw1].astype(np.float32), Tcw2=np.c_[Rw2, tw2].astype(np.float32),
                K4_1=K4, K4_2=K4, m12=m12, level_sigma2=LEVEL_SIGMA2, fix_scale=bool(fix_scale),
                s12=float(s), R12=R21.T.copy(), t12=-R21.T @ t21, good=good, extent=float(np.ptp(Xc1, axis=0).max()))


def case_scene(c, seed=0):
    return scene(c[0], c[1], c[2], c[3], seed=seed)


def words(iterations, seed):
    """iterations * 3 rand()-like words (0 .. 2^31 - 1), seeded: the parity tests feed the same words to both sides."""
    return np.random.default_rng(20_000 + seed).integers(0, 2 ** 31, iterations * 3, dtype=np.int64).astype(np.int32)


# the words of a case: seeded by N, except where that draw puts a hypothesis with close leading eigenvalues (one the parity contract
# does not compare) before the winner of a case whose decision the contract wants compared
_WORD_SEED = {(1000, 0.7, 0.3, False): 1001, (1000, 1.0, 0.3, True): 1001}


def case_words(c):
    return words(ransac_of(c)[2], _WORD_SEED.get(tuple(c), c[0]))
