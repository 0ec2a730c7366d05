"""The marker-pose inputs of tests/golden/pose_hard_cases.npz, by family: seeded, numpy only (no reference, no mpmath), so that the
generator, the CPU test and the GPU test's larger fronto-parallel samples all draw the same corners.  A case is (corners float32 (4, 2),
R, t of the true pose or None); a family carries its camera (K4, distortion vector) and marker side."""
import numpy as np

import pose_cases as pc

DIST12 = np.array([0.12, -0.25, -0.0012, 0.0021, 0.08, 0.05, -0.02, 0.01, 0.0015, -0.0008, 0.0011, 0.0006], np.float32)
NODIST = np.zeros(0, np.float32)
K_GRID = np.array([500, 500, 320, 240], np.float32)
GRID_SQUARE = np.array([[270, 190], [370, 190], [370, 290], [270, 290]], np.float32)
SIZE = 0.187


def project12(P, R, t, K, d):
    """forward model in float64 with all twelve coefficients (rational and thin prism included): P n x 3 -> pixels"""
    k = np.zeros(12); d = np.asarray(d, np.float64).ravel(); k[:len(d)] = d
    X = (R @ np.asarray(P, np.float64).T).T + t
    x = X[:, 0] / X[:, 2]; y = X[:, 1] / X[:, 2]
    r2 = x * x + y * y
    cd = (1 + k[0] * r2 + k[1] * r2 ** 2 + k[4] * r2 ** 3) / (1 + k[5] * r2 + k[6] * r2 ** 2 + k[7] * r2 ** 3)
    xd = x * cd + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 ** 2
    yd = y * cd + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 ** 2
    return np.stack([xd * float(K[0]) + float(K[2]), yd * float(K[1]) + float(K[3])], 1)


def camera_resize(K4, cam_size, img_size):
    """CameraParameters::resize in float, as orbfe_camera_resize computes it"""
    ax, ay = np.float32(img_size[0]) / np.float32(cam_size[0]), np.float32(img_size[1]) / np.float32(cam_size[1])
    return np.array([K4[0] * ax, K4[1] * ay, K4[2] * ax, K4[3] * ay], np.float32)


def placed(n, seed, tilt, K4, dist, size=SIZE, depth=(0.5, 2.5), box=(5, 5, 635, 475), behind=False, inplane=np.pi):
    """n markers tilted by `tilt` rad (about a random axis in the image plane) from facing the camera, at a random in-plane angle and
    position (the in-plane angle within +-inplane), all corners inside `box`.  behind: the marker's back faces the camera (rotation near the identity, corner order reversed)."""
    rng = np.random.default_rng(seed)
    P = pc.object_points(size)
    out = []
    while len(out) < n:
        a = rng.uniform(-np.pi, np.pi)
        R = pc.rodrigues(np.array([np.cos(a), np.sin(a), 0]) * tilt) @ pc.rodrigues([0 if behind else np.pi, 0, 0]) @ pc.rodrigues([0, 0, rng.uniform(-inplane, inplane)])
        z = rng.uniform(*depth)
        t = np.array([rng.uniform(-0.7, 0.7) * z, rng.uniform(-0.5, 0.5) * z, z])
        c = project12(P, R, t, K4, dist)
        if c[:, 0].min() < box[0] or c[:, 1].min() < box[1] or c[:, 0].max() > box[2] or c[:, 1].max() > box[3]:
            continue
        out.append((c.astype(np.float32), R, t))
    return out


def families():
    """-> list of {name, K4, dist, size, cases, degenerate, fronto}"""
    K4 = pc.K4
    F = []

    def add(name, cases, K=K4, dist=pc.DIST, size=SIZE, degenerate=False, fronto=False, seed=None):
        F.append({"name": name, "seed": seed, "K4": np.asarray(K, np.float32), "dist": np.asarray(dist, np.float32), "size": float(size), "cases": cases,
                  "degenerate": degenerate, "fronto": fronto})

    add("fronto_dist", placed(48, 101, 0.0, K4, pc.DIST), fronto=True, seed=101)
    add("fronto_nodist", placed(48, 102, 0.0, K4, NODIST), dist=NODIST, fronto=True, seed=102)
    # two fronto-parallel records on which the oracle's rot2vec has no value for the true solution (trace below -1): the 58th and 256th draw
    wide = placed(256, 101, 0.0, K4, pc.DIST)
    add("fronto_half_turn", [wide[57], wide[255]])
    for i, tilt in enumerate((1e-4, 1e-3, 1e-2, 5e-2)):
        add("near_fronto_%g" % tilt, placed(20, 110 + i, tilt, K4, NODIST if i % 2 else pc.DIST), dist=NODIST if i % 2 else pc.DIST)
    add("steep_1.3", placed(20, 120, 1.3, K4, NODIST), dist=NODIST)
    add("steep_1.5", placed(20, 121, 1.5, K4, NODIST), dist=NODIST)
    grid = [(np.roll(GRID_SQUARE + np.float32(s), -k, axis=0), None, None) for s in ((0, 0), (37, -21)) for k in range(4)]
    add("pixel_grid", grid, K=K_GRID, dist=NODIST, size=0.2)
    add("coef8", placed(20, 130, 0.6, K4, DIST12[:8]) + placed(4, 131, 0.0, K4, DIST12[:8]), dist=DIST12[:8])
    add("coef12", placed(20, 132, 0.6, K4, DIST12) + placed(4, 133, 0.0, K4, DIST12), dist=DIST12)
    add("behind", placed(8, 140, 0.02, K4, NODIST, behind=True, inplane=0.02) + placed(8, 141, 0.3, K4, NODIST, behind=True, inplane=0.1)
        + placed(8, 142, 1e-3, K4, NODIST, behind=True, inplane=1e-3),
        dist=NODIST)
    Kw = np.array([K4[0], 2 * K4[1], K4[2], K4[3]], np.float32)
    add("cam_fx_fy", placed(12, 150, 0.5, Kw, pc.DIST), K=Kw)
    Kr = camera_resize(K4, (1280, 720), (640, 480))
    add("cam_resized", placed(12, 151, 0.5, Kr, pc.DIST, box=(5, 5, 315, 315)), K=Kr)
    add("size_1e-3", placed(12, 152, 0.4, K4, pc.DIST, size=1e-3, depth=(0.5e-3 / SIZE, 2.5e-3 / SIZE)), size=1e-3)
    add("size_100", placed(12, 153, 0.4, K4, pc.DIST, size=100, depth=(50 / SIZE, 250 / SIZE)), size=100)
    add("px_1.5", placed(12, 154, 0.3, K4, pc.DIST, depth=(60, 68)))
    add("outside", placed(12, 155, 0.4, K4, NODIST, depth=(0.08, 0.14), box=(-400, -300, 1000, 800)), dist=NODIST)
    q = placed(1, 160, 0.5, K4, pc.DIST)[0][0]
    deg = [np.repeat(q[:1], 4, 0), q[[0, 0, 2, 2]], np.array([[100, 100], [150, 125], [200, 150], [300, 200]], np.float32), q[[0, 2, 1, 3]]]
    add("degenerate", [(np.ascontiguousarray(c, np.float32), None, None) for c in deg], degenerate=True)
    return F


DEGENERATE_NAMES = ("four_equal", "two_pairs", "collinear", "bow_tie")


def fronto_sample(n, seed, with_dist):
    """a larger fronto-parallel sample for the NaN share: corners (n, 4, 2) float32, and its camera"""
    d = pc.DIST if with_dist else NODIST
    return np.stack([c for c, _, _ in placed(n, seed, 0.0, pc.K4, d)]), pc.K4, d
