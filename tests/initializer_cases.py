"""Seeded synthetic two-view scenes for the Initializer tests: 3D points seen by two pinhole cameras (K, known R, t), sigma = 1 px
keypoint noise, a share of outlier matches, and unmatched keypoints in both frames (so that Normalize() runs over more points than
the matches, as in the reference)."""
import numpy as np

from oracle_lib import KP_DTYPE  # noqa: F401  (the scene modules take it from here)
K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]], np.float32)
COLS, ROWS = 640, 480


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _project(P, R, t):
    Xc = P @ R.T + t
    uv = Xc[:, :2] / Xc[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    return uv, Xc[:, 2]


def _kps(uv, rng):
    k = np.zeros(len(uv), KP_DTYPE)
    k["x"], k["y"] = uv[:, 0], uv[:, 1]
    k["size"] = 31; k["angle"] = rng.uniform(0, 360, len(uv)); k["response"] = rng.uniform(0, 1e-3, len(uv))
    k["octave"] = rng.integers(0, 8, len(uv)); k["class_id"] = -1
    return k


def scene(kind, n, outliers=0.0, seed=0, noise=1.0, extra=20):
    """kind: 'planar' (H branch), 'general' (3D structure, wide baseline: F branch), 'rotation' (no translation: no initialization).
    Returns dict(kps1, kps2, m12, R, t, X) with X the true points of frame-1 keypoints (NaN for outliers / unmatched)."""
    rng = np.random.default_rng(seed)
    if kind == "planar":
        R, t = rot([0.2, 1, 0.1], 6.0), np.array([-0.6, 0.1, 0.05])
    elif kind == "general":
        R, t = rot([0.1, 1, 0.05], 8.0), np.array([-1.5, 0.1, 0.1])
    elif kind == "rotation":
        R, t = rot([0.3, 1, 0.1], 4.0), np.zeros(3)
    else:
        raise ValueError(kind)
    P = []
    while sum(len(p) for p in P) < n:
        m = 4 * n + 64
        uv = np.stack([rng.uniform(10, COLS - 10, m), rng.uniform(10, ROWS - 10, m)], 1)
        if kind == "planar":   # the plane z = 6 + 0.15 x
            ray = np.c_[(uv - [K[0, 2], K[1, 2]]) / [K[0, 0], K[1, 1]], np.ones(m)]
            z = 6.0 / (1 - 0.15 * ray[:, 0])
        else:
            z = rng.uniform(3.0, 8.0, m)
            ray = np.c_[(uv - [K[0, 2], K[1, 2]]) / [K[0, 0], K[1, 1]], np.ones(m)]
        X = ray * z[:, None]
        uv2, z2 = _project(X, R, t)
        ok = (z2 > 0.5) & (uv2[:, 0] > 5) & (uv2[:, 0] < COLS - 5) & (uv2[:, 1] > 5) & (uv2[:, 1] < ROWS - 5)
        P.append(X[ok])
    X = np.concatenate(P)[:n]
    uv1, _ = _project(X, np.eye(3), np.zeros(3))
    uv2, _ = _project(X, R, t)
    uv1 = uv1 + rng.normal(0, noise, uv1.shape); uv2 = uv2 + rng.normal(0, noise, uv2.shape)
    nout = int(round(outliers * n))
    bad = rng.choice(n, nout, replace=False)
    uv2[bad] = np.stack([rng.uniform(5, COLS - 5, nout), rng.uniform(5, ROWS - 5, nout)], 1)
    # frame 1: the n matched keypoints shuffled among `extra` unmatched ones; frame 2 the same with its own order
    n1, n2 = n + extra, n + extra
    pos1 = rng.permutation(n1)[:n]; pos2 = rng.permutation(n2)[:n]
    all1 = np.stack([rng.uniform(5, COLS - 5, n1), rng.uniform(5, ROWS - 5, n1)], 1)
    all2 = np.stack([rng.uniform(5, COLS - 5, n2), rng.uniform(5, ROWS - 5, n2)], 1)
    all1[pos1] = uv1; all2[pos2] = uv2
    m12 = np.full(n1, -1, np.int32); m12[pos1] = pos2
    Xt = np.full((n1, 3), np.nan); Xt[pos1] = X
    Xt[pos1[bad]] = np.nan
    return dict(kps1=_kps(all1, rng), kps2=_kps(all2, rng), m12=m12, R=R.astype(np.float32), t=t.astype(np.float32), X=Xt)


def words(iterations, seed):
    """iterations * 8 rand()-like words (0 .. 2^31 - 1), seeded: the parity tests feed the same words to both sides."""
    return np.random.default_rng(10_000 + seed).integers(0, 2 ** 31, iterations * 8, dtype=np.int64).astype(np.int32)
