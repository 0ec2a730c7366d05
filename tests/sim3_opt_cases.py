"""Seeded problems for the OptimizeSim3 tests: the loop-closure scenes of tests/sim3_cases.py (two keyframes whose maps differ by a
known similarity, pixel noise, a share of gross outliers) with an initial similarity next to the truth, as the Sim3 RANSAC hands
it over: rotated by `deg` degrees, shifted by `shift` of the scene extent and, where the scale is free, scaled by `dscale`.
th2 = 10 is the loop closer's (LoopClosing.cc:425, :580).  inv_sigma2 = 1 / level_sigma2 of the scenes."""
import numpy as np

import sim3_cases
from initializer_cases import rot

TH2 = 10.0
INV_SIGMA2 = (np.float32(1.0) / sim3_cases.LEVEL_SIGMA2).astype(np.float32)

# name: (N, true scale, outliers (a count when >= 1, else a share of N), fix_scale, valid arrays given, noise in pixels, seed)
CASES = {
    "n0": (0, 1.0, 0, True, True, 1.0, 0),
    "n9_clean": (9, 1.3, 0, False, True, 0.0, 0),
    "n10_clean_fix": (10, 1.0, 0, True, True, 0.0, 0),
    "n10_one_outlier": (10, 1.0, 1, True, True, 0.3, 0),
    "n11_one_outlier": (11, 1.3, 1, False, True, 0.3, 0),
    "n64_free": (64, 0.7, 0, False, True, 1.0, 0),
    "n64_fix_novalid": (64, 1.0, 0.3, True, False, 1.0, 0),
    "n100_clean_s07": (100, 0.7, 0, False, True, 0.0, 0),
    "n100_clean_s1": (100, 1.0, 0, False, False, 0.0, 0),
    "n100_clean_s13_fix": (100, 1.3, 0, True, True, 0.0, 0),
    "n100_clean_s07_fix": (100, 0.7, 0, True, True, 0.0, 0),
    "n257_out30": (257, 1.3, 0.3, False, True, 1.0, 0),
    "n257_fix": (257, 1.0, 0, True, False, 1.0, 0),
    "n300_out60": (300, 1.0, 0.6, True, True, 1.0, 0),
    "n300_free_out30_novalid": (300, 0.7, 0.3, False, False, 1.0, 0),
    "n300_out60_free": (300, 1.3, 0.6, False, True, 0.5, 0),
    "n1000_out30": (1000, 1.3, 0.3, False, True, 1.0, 0),
    "n1000_fix": (1000, 1.0, 0, True, True, 1.0, 0),
    "n1000_out60_novalid": (1000, 1.0, 0.6, False, False, 1.0, 0),
    "n40_noisy": (40, 1.0, 0.3, False, True, 2.0, 0),
    "n20_noisy_fix": (20, 1.0, 0.3, True, True, 2.0, 0),
    "n30_far_start": (30, 1.3, 0.3, False, True, 1.5, 0),
}
# the start of a case: (degrees, shift as a share of the extent, relative scale step)
START = {"n30_far_start": (4.0, 0.05, 0.10)}
CLEAN = [n for n, c in CASES.items() if c[5] == 0.0 and c[2] == 0 and c[0] >= 10]


def problem(N, s=1.0, outliers=0.0, fix_scale=False, with_valid=True, noise=1.0, seed=0, start=(1.0, 0.01, 0.03)):
    empty = N == 0
    n = 20 if empty else N
    share = outliers / n if outliers >= 1 else outliers
    sc = sim3_cases.scene(n, s, share, fix_scale, seed=seed, noise=noise, dropped=5 if with_valid else 0)
    rng = np.random.default_rng(77_000 + 1000 * seed + N)
    deg, shift, dscale = start
    R0 = rot(rng.normal(size=3), deg) @ sc["R12"]
    t0 = sc["t12"] + rng.normal(size=3) * shift * sc["extent"] / np.sqrt(3.0)
    s0 = sc["s12"] if fix_scale else sc["s12"] * (1.0 + dscale)
    m12 = np.full_like(sc["m12"], -1) if empty else sc["m12"]
    return dict(kps1=sc["kps1"], kps2=sc["kps2"], x3Dw1=sc["x3Dw1"], x3Dw2=sc["x3Dw2"],
                valid1=sc["valid1"] if with_valid else None, valid2=sc["valid2"] if with_valid else None,
                Tcw1=sc["Tcw1"], Tcw2=sc["Tcw2"], K4_1=sc["K4_1"], K4_2=sc["K4_2"], m12=m12, inv_sigma2=INV_SIGMA2,
                s12_0=np.float32(s0), R12_0=R0.astype(np.float32), t12_0=t0.astype(np.float32), th2=TH2, fix_scale=bool(fix_scale),
                s12=sc["s12"], R12=sc["R12"], t12=sc["t12"], good=sc["good"] & (not empty), extent=sc["extent"], N=N)


def case(name):
    c = CASES[name]
    return problem(c[0], c[1], c[2], c[3], c[4], c[5], c[6], START.get(name, (1.0, 0.01, 0.03)))


def degenerate_problem(ngood, nzero, seed=0):
    """Finite inputs whose projections divide by z = 0: both keyframes sit at their maps' origins, the true and the initial similarity
    are the identity, `ngood` pairs are ordinary points (0.5 px of observation noise) and `nzero` pairs have z = 0 in both maps, so at
    the initial estimate e12 and e21 of such a pair are inf / NaN.  The degenerate pairs come first.  The scale is fixed: two cameras at
    one place do not observe it."""
    rng = np.random.default_rng(88_000 + seed)
    n = ngood + nzero
    K4 = sim3_cases.K4
    X = sim3_cases._cloud(rng, n)
    X[:nzero, 2] = 0.0
    uv = np.full((n, 2), 100.0)
    uv[nzero:] = sim3_cases._image(X[nzero:])
    k1 = sim3_cases._kps(uv + rng.normal(0, 0.5, (n, 2)), rng); k2 = sim3_cases._kps(uv + rng.normal(0, 0.5, (n, 2)), rng)
    k1["octave"] = 0; k2["octave"] = 0
    T = np.c_[np.eye(3), np.zeros(3)].astype(np.float32)
    good = np.ones(n, bool); good[:nzero] = False
    return dict(kps1=k1, kps2=k2, x3Dw1=X.astype(np.float32), x3Dw2=X.astype(np.float32), valid1=None, valid2=None, Tcw1=T, Tcw2=T,
                K4_1=K4, K4_2=K4, m12=np.arange(n, dtype=np.int32), inv_sigma2=INV_SIGMA2, s12_0=np.float32(1.0),
                R12_0=np.eye(3, dtype=np.float32), t12_0=np.zeros(3, np.float32), th2=TH2, fix_scale=True, s12=1.0, R12=np.eye(3),
                t12=np.zeros(3), good=good, extent=float(np.ptp(X[nzero:], axis=0).max()) if ngood else 1.0, N=n)


def rotation_of(q):
    """The rotation matrix of a quaternion (x, y, z, w) as Eigen's toRotationMatrix gives it (no normalisation)."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def similarity_difference(ra, rb, extent):
    """(max |dR|, |ds| / s, |dt| / extent) between two result records."""
    dR = np.abs(rotation_of(ra["q12"]) - rotation_of(rb["q12"])).max()
    return float(dR), float(abs(ra["s12"] - rb["s12"]) / abs(rb["s12"])), float(np.abs(ra["t12"] - rb["t12"]).max() / extent)
