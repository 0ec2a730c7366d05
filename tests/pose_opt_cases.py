"""Seeded synthetic problems for the pose optimization tests: map points in front of a camera at a known pose, keypoints with
1 px noise scaled by the octave's scale factor, a share of gross outliers, keypoints without map points, ArUco markers with a known
Twm, and an initial pose a few degrees and centimetres off (or exactly the true one, noise-free)."""
import numpy as np

from pose_opt_build import KP_DTYPE, MARKER_DTYPE

K4 = np.array([500.0, 500.0, 320.0, 240.0], np.float32)
COLS, ROWS = 640, 480
NLEVELS, SCALE = 8, 1.2
INV_SIGMA2 = np.array([1.0 / SCALE ** (2 * l) for l in range(NLEVELS)], np.float32)
DEPTH = 5.0          # the scenes' typical depth (the parity tolerance of t is relative to it)
MARKER_SIDE = 0.2


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(Tcw, Xw):
    Xc = Xw @ Tcw[:, :3].T + Tcw[:, 3]
    return Xc[:, :2] / Xc[:, 2:3] * K4[:2] + K4[2:], Xc[:, 2]


def local_corners(side=MARKER_SIDE):
    h = side / 2
    return np.array([[-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0]], np.float64)


def problem(n, outliers=0.0, nmarkers=0, seed=0, noise=1.0, perturb=(2.0, 0.05), unmatched=0.1):
    """n keypoints with a map point (plus round(unmatched * n) without), `outliers` of them gross; nmarkers markers; the initial pose
    perturbed by perturb = (degrees, metres).  Returns the problem dict the builders and the bindings take, plus the ground truth
    (T_true, bad: the injected outliers, depth)."""
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(0, 30))
    t = rng.normal(size=3) * 0.5
    T_true = np.concatenate([R, t[:, None]], 1)
    # map points: a pixel and a depth, back to the world
    uv = rng.uniform([10, 10], [COLS - 10, ROWS - 10], (n, 2))
    z = rng.uniform(0.5 * DEPTH, 1.5 * DEPTH, n)
    Xc = np.concatenate([(uv - K4[2:]) / K4[:2] * z[:, None], z[:, None]], 1)
    Xw = (Xc - t) @ R
    oct_ = rng.integers(0, NLEVELS, n)
    obs = uv + rng.normal(size=(n, 2)) * noise * (SCALE ** oct_)[:, None]
    bad = np.zeros(n, bool)
    nb = int(round(outliers * n))
    if nb:
        idx = rng.choice(n, nb, replace=False)
        bad[idx] = True
        shift = rng.uniform(20, 120, (nb, 2)) * rng.choice([-1, 1], (nb, 2))
        obs[idx] = np.clip(obs[idx] + shift, 0, [COLS, ROWS])
    # keypoints without a map point, interleaved
    nu = int(round(unmatched * n))
    order = rng.permutation(n + nu)
    kps = np.zeros(n + nu, KP_DTYPE)
    has = np.zeros(n + nu, np.uint8)
    X = np.zeros((n + nu, 3), np.float32)
    badk = np.zeros(n + nu, bool)
    src = order < n
    kps["x"][src] = obs[order[src], 0]; kps["y"][src] = obs[order[src], 1]
    kps["octave"][src] = oct_[order[src]]
    has[src] = 1
    X[src] = Xw[order[src]]
    badk[src] = bad[order[src]]
    kps["x"][~src] = rng.uniform(0, COLS, (~src).sum()); kps["y"][~src] = rng.uniform(0, ROWS, (~src).sum())
    kps["octave"][~src] = rng.integers(0, NLEVELS, (~src).sum())
    kps["size"] = 31; kps["angle"] = rng.uniform(0, 360, n + nu); kps["response"] = 1e-3; kps["class_id"] = -1
    # markers: squares facing the camera, at a pixel and a depth
    mk = np.zeros(nmarkers, MARKER_DTYPE)
    L = local_corners()
    for m in range(nmarkers):
        c = rng.uniform([120, 100], [COLS - 120, ROWS - 100])
        zc = rng.uniform(0.4 * DEPTH, 0.8 * DEPTH)
        pc = np.array([(c[0] - K4[2]) / K4[0] * zc, (c[1] - K4[3]) / K4[1] * zc, zc])
        Rcm = rot([1, 0, 0], 180) @ rot(rng.normal(size=3), rng.uniform(0, 25))  # marker z towards the camera
        Rwm = R.T @ Rcm
        twm = R.T @ (pc - t)
        Twm = np.concatenate([Rwm, twm[:, None]], 1)
        Pw = L @ Rwm.T + twm
        cuv, _ = project(T_true, Pw)
        cuv = cuv + rng.normal(size=(4, 2)) * 0.5 * noise
        mk[m]["corners"] = cuv.reshape(8)
        mk[m]["Twm"] = Twm.reshape(12).astype(np.float32)
        mk[m]["local"] = L.reshape(12).astype(np.float32)
    dR = rot(rng.normal(size=3), perturb[0])
    dt = rng.normal(size=3); dt = dt / np.linalg.norm(dt) * perturb[1]
    T0 = np.concatenate([dR @ R, (dR @ t + dt)[:, None]], 1)
    return dict(kps=kps, has_mp=has, x3Dw=X, inv_sigma2=INV_SIGMA2, K4=K4, markers=mk, marker_info=25.0,
                Tcw=T0.astype(np.float32), T_true=T_true, bad=badk, depth=DEPTH)


# name -> problem(...) arguments.  Across them: gross outliers 0 / 10 / 30 / 50 %, 0 / 1 / 3 markers, sizes 2 .. 2000, a
# marker-dominated scene, and noise-free scenes that start at the true pose (rounds that end on rejected trials).
CASES = {
    "n2": dict(n=2, seed=1),
    "n2_markers": dict(n=2, nmarkers=3, seed=2),
    "n5": dict(n=5, seed=3),
    "n5_marker": dict(n=5, nmarkers=1, seed=4),
    "n9": dict(n=9, seed=5),
    "n9_out10": dict(n=9, outliers=0.1, seed=6),
    "n60": dict(n=60, seed=7),
    "n60_out30_m1": dict(n=60, outliers=0.3, nmarkers=1, seed=8),
    "n60_out50": dict(n=60, outliers=0.5, seed=9),
    "n500": dict(n=500, seed=10),
    "n500_out10_m3": dict(n=500, outliers=0.1, nmarkers=3, seed=11),
    "n500_out30": dict(n=500, outliers=0.3, seed=12),
    "n500_out50_m1": dict(n=500, outliers=0.5, nmarkers=1, seed=13),
    "n2000_out10": dict(n=2000, outliers=0.1, seed=14),
    "n2000_out30_m3": dict(n=2000, outliers=0.3, nmarkers=3, seed=15),
    "n1000_m2": dict(n=1000, outliers=0.1, nmarkers=2, seed=16),
    "marker_dominated": dict(n=6, outliers=0.0, nmarkers=3, seed=17),
    "marker_dominated_out": dict(n=12, outliers=0.3, nmarkers=3, seed=18),
    "big_perturb": dict(n=300, outliers=0.1, nmarkers=1, seed=19, perturb=(6.0, 0.15)),
    "clean_true_n60": dict(n=60, seed=20, noise=0.0, perturb=(0.0, 0.0)),
    "clean_true_n500_m1": dict(n=500, nmarkers=1, seed=21, noise=0.0, perturb=(0.0, 0.0)),
    "clean_true_n9": dict(n=9, seed=22, noise=0.0, perturb=(0.0, 0.0)),
    "clean_true_n2000_m3": dict(n=2000, nmarkers=3, seed=23, noise=0.0, perturb=(0.0, 0.0)),
    "clean_n500": dict(n=500, seed=24, noise=0.0),
}


def case(name):
    return problem(**CASES[name])
