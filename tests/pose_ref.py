"""A high-precision statement of the marker pose solver (csrc/aruco_pose.hpp), stage by stage and as a whole, for
tests/gen_pose_golden.py and tests/test_pose_ref_cpu.py.  The GPU tests never import this module: they read the fixture it writes.

Every function takes an arithmetic `M`: MP (mpmath at 50 digits) is the reference, F64 (numpy doubles, LAPACK for the linear solves) is
the plain double evaluation whose error against MP sets the stage bounds.  Values are rounded to float exactly where the code rounds:
the normalised corners (cv::undistortPoints' CV_32FC2 result) and, in reprojection_error_float, the projected points and the float sums
of evalReprojError.  What is cheap to state independently is: the homography is the exact 8 x 8 solve of the four correspondences (the
HO estimator's result for four points, which fit exactly), the translation solves its 3 x 3 normal equations by elimination, the
eigenvector comes from mpmath.eigsy, the rotation vector from a logarithm that is well conditioned at a half turn."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = 2.0 ** -52
FLT_EPS = 2.0 ** -23


class MP:
    num = staticmethod(mp.mpf)
    sqrt, acos, sin, cos, atan2 = (staticmethod(f) for f in (mp.sqrt, mp.acos, mp.sin, mp.cos, mp.atan2))

    @staticmethod
    def solve(A, b):
        return list(mp.lu_solve(mp.matrix(A), mp.matrix(b)))


class F64:
    num = staticmethod(np.float64)
    sqrt, acos, sin, cos, atan2 = (staticmethod(f) for f in (np.sqrt, np.arccos, np.sin, np.cos, np.arctan2))

    @staticmethod
    def solve(A, b):
        return list(np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64)))


def camera(K4, dist):
    """the PoseCamera of pose_camera(): float inputs widened to double"""
    d = np.asarray(dist, np.float32).ravel()
    k = np.zeros(12)
    k[:len(d)] = d
    K4 = np.asarray(K4, np.float32)
    return {"fx": float(K4[0]), "fy": float(K4[1]), "cx": float(K4[2]), "cy": float(K4[3]), "k": [float(v) for v in k], "has_dist": int(len(d) > 0)}


def camera17(cam):
    """fx fy cx cy k[12] has_dist as 17 doubles: what the probe's calls take"""
    return np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]] + cam["k"] + [cam["has_dist"]], np.float64)


def f32(x):
    return float(np.float32(float(x)))


def object_points(size):
    h = float(np.float32(size) / np.float32(2))
    return [(-h, h), (h, h), (h, -h), (-h, -h)]


# ------------------------------------------------------------------------------------------------------------------------ stages
def normalise_point(M, u, v, cam, rounded=True):
    n = M.num
    x = (n(float(u)) - n(cam["cx"])) * (1 / n(cam["fx"])); y = (n(float(v)) - n(cam["cy"])) * (1 / n(cam["fy"]))
    if cam["has_dist"]:
        k = [n(c) for c in cam["k"]]
        x0, y0 = x, y
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            dX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            dY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = (x0 - dX) * icdist; y = (y0 - dY) * icdist
    return (f32(x), f32(y)) if rounded else (x, y)


def dlt_rows(src, dst):
    """the 8 x 8 system of H(2,2) = 1 for four correspondences src -> dst"""
    A, b = [], []
    for (X, Y), (u, v) in zip(src, dst):
        A.append([X, Y, 1, 0, 0, 0, -u * X, -u * Y]); b.append(u)
        A.append([0, 0, 0, X, Y, 1, -v * X, -v * Y]); b.append(v)
    return A, b


def homography(M, src, dst):
    n = M.num
    A, b = dlt_rows([(n(x), n(y)) for x, y in src], [(n(x), n(y)) for x, y in dst])
    return M.solve(A, b) + [n(1)]


def homography_condition(src, dst):
    A, _ = dlt_rows(src, dst)
    return float(np.linalg.cond(np.array(A, np.float64), np.inf))


def jacobian(H):
    return [H[0] - H[6] * H[2], H[1] - H[7] * H[2], H[3] - H[6] * H[5], H[4] - H[7] * H[5], H[2], H[5]]


def rotations(M, j6):
    """-> R1, R2 (9 each, row-major), the two radicands of computeRotations"""
    n = M.num
    j00, j01, j10, j11, p, q = [n(v) for v in j6]
    nrm = M.sqrt(p * p + q * q + 1)
    ax, ay, az = p / nrm, q / nrm, 1 / nrm
    d = 1 / (1 + az)
    Ra = [[1 - ax * ax * d, -ax * ay * d, -ax], [-ax * ay * d, 1 - ay * ay * d, -ay], [ax, ay, 1 - (ax * ax + ay * ay) * d]]
    rv = [[Ra[c][r] for c in range(3)] for r in range(3)]
    b00, b01, b10, b11 = rv[0][0] - p * rv[2][0], rv[0][1] - p * rv[2][1], rv[1][0] - q * rv[2][0], rv[1][1] - q * rv[2][1]
    dt = b00 * b11 - b01 * b10
    a00, a01 = (b11 * j00 - b01 * j10) / dt, (b11 * j01 - b01 * j11) / dt
    a10, a11 = (-b10 * j00 + b00 * j10) / dt, (-b10 * j01 + b00 * j11) / dt
    s00, s01, s11 = a00 * a00 + a01 * a01, a00 * a10 + a01 * a11, a10 * a10 + a11 * a11
    gamma = M.sqrt((s00 + s11 + M.sqrt((s00 - s11) ** 2 + 4 * s01 * s01)) / 2)
    r00, r01, r10, r11 = a00 / gamma, a01 / gamma, a10 / gamma, a11 / gamma
    rad0, rad1 = 1 - r00 * r00 - r10 * r10, 1 - r01 * r01 - r11 * r11
    if M is MP:      # gamma is the larger singular value, so both are >= 0 exactly; 50 digits may leave -1e-50
        c0, c1 = max(rad0, n(0)), max(rad1, n(0))
    else:
        c0, c1 = rad0, rad1
    b0, b1 = M.sqrt(c0), M.sqrt(c1)
    if -r00 * r01 - r10 * r11 < 0:
        b1 = -b1
    out = []
    for sg in (1, -1):
        c0v, c1v = (r00, r10, sg * b0), (r01, r11, sg * b1)
        c2v = (c0v[1] * c1v[2] - c0v[2] * c1v[1], c0v[2] * c1v[0] - c0v[0] * c1v[2], c0v[0] * c1v[1] - c0v[1] * c1v[0])
        R = []
        for i in range(3):
            for col in (c0v, c1v, c2v):
                R.append(rv[i][0] * col[0] + rv[i][1] * col[1] + rv[i][2] * col[2])
        out.append(R)
    return out[0], out[1], rad0, rad1


def translation(M, obj, img, R):
    """least squares of  t_x - u t_z = u rz - rx,  t_y - v t_z = v rz - ry  over the four points, by its normal equations"""
    n = M.num
    R = [n(v) for v in R]
    AtA = [[n(0)] * 3 for _ in range(3)]
    Atb = [n(0)] * 3
    for (X, Y), (u, v) in zip(obj, img):
        X, Y, u, v = n(X), n(Y), n(u), n(v)
        rx, ry, rz = R[0] * X + R[1] * Y, R[3] * X + R[4] * Y, R[6] * X + R[7] * Y
        for row, rhs in (((n(1), n(0), -u), u * rz - rx), ((n(0), n(1), -v), v * rz - ry)):
            for a in range(3):
                Atb[a] = Atb[a] + row[a] * rhs
                for b in range(3):
                    AtA[a][b] = AtA[a][b] + row[a] * row[b]
    return M.solve(AtA, Atb)


def translation_condition(img):
    a = np.array(img, np.float64)
    AtA = np.array([[4, 0, -a[:, 0].sum()], [0, 4, -a[:, 1].sum()], [-a[:, 0].sum(), -a[:, 1].sum(), (a ** 2).sum()]])
    return float(np.linalg.cond(AtA, np.inf))


def rodrigues(M, r):
    n = M.num
    r = [n(v) for v in r]
    th = M.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if th == 0:
        return [n(int(i % 4 == 0)) for i in range(9)]
    x, y, z = r[0] / th, r[1] / th, r[2] / th
    c, s = M.cos(th), M.sin(th)
    c1 = 1 - c
    return [c + c1 * x * x, c1 * x * y - s * z, c1 * x * z + s * y, c1 * x * y + s * z, c + c1 * y * y, c1 * y * z - s * x,
            c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z]


def rot2vec(M, R):
    """PoseSolver::rot2vec as written (ippe.cpp:368-397): w / (2 sin w) times the skew part; zero below FLT_EPSILON"""
    n = M.num
    R = [n(v) for v in R]
    w = M.acos((R[0] + R[4] + R[8] - 1) / 2)
    if w < FLT_EPS:
        return [n(0)] * 3, w
    d = 1 / (2 * M.sin(w)) * w
    return [d * (R[7] - R[5]), d * (R[2] - R[6]), d * (R[3] - R[1])], w


def log_rotation(R):
    """the rotation vector of an (mp) rotation matrix, well conditioned up to and at a half turn: the angle from atan2 of the skew part's
    length and the trace, the axis from the skew part, or from the largest column of R + I where the skew part vanishes"""
    R = [mp.mpf(v) for v in R]
    k = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    s = mp.sqrt(k[0] ** 2 + k[1] ** 2 + k[2] ** 2) / 2
    w = mp.atan2(s, (R[0] + R[4] + R[8] - 1) / 2)
    if w == 0:
        return [mp.mpf(0)] * 3, w
    if s > mp.mpf(10) ** -20:
        return [v / (2 * s) * w for v in k], w
    S = [[(R[3 * i + j] + R[3 * j + i]) / 2 + (1 if i == j else 0) for j in range(3)] for i in range(3)]     # (1 - cos w) a a^T + ...
    c = max(range(3), key=lambda j: S[j][j])
    a = [S[i][c] for i in range(3)]
    nrm = mp.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2)
    a = [v / nrm for v in a]
    if a[0] * k[0] + a[1] * k[1] + a[2] * k[2] < 0:
        a = [-v for v in a]
    return [v * w for v in a], w


def project_point(M, X, Y, R, t, cam):
    """cv::projectPoints of (X, Y, 0): pixel coordinates, not rounded; the z == 0 guard as in the code"""
    n = M.num
    k = [n(c) for c in cam["k"]]
    x = R[0] * X + R[1] * Y + t[0]; y = R[3] * X + R[4] * Y + t[1]; z = R[6] * X + R[7] * Y + t[2]
    z = 1 / z if z != 0 else n(1)
    x = x * z; y = y * z
    r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
    a1, a2, a3 = 2 * x * y, r2 + 2 * x * x, r2 + 2 * y * y
    cd = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6
    icd2 = 1 / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6)
    xd = x * cd * icd2 + k[2] * a1 + k[3] * a2 + k[8] * r2 + k[9] * r4
    yd = y * cd * icd2 + k[2] * a3 + k[3] * a1 + k[10] * r2 + k[11] * r4
    return xd * n(cam["fx"]) + n(cam["cx"]), yd * n(cam["fy"]) + n(cam["cy"])


def reprojection_rms(M, obj, corners, cam, R, t):
    """the reprojection RMS of the rotation matrix itself, nothing rounded"""
    n = M.num
    R, t = [n(v) for v in R], [n(v) for v in t]
    e = n(0)
    for (X, Y), (u, v) in zip(obj, corners):
        pu, pv = project_point(M, n(X), n(Y), R, t, cam)
        e = e + (pu - n(float(u))) ** 2 + (pv - n(float(v))) ** 2
    return M.sqrt(e / 8)


def reprojection_error_float(M, obj, corners, cam, R, t):
    """evalReprojError as the code rounds it: rot2vec, Rodrigues (identity below DBL_EPSILON), projections rounded to float, float
    differences and float sums, sqrtf"""
    n = M.num
    r, _ = rot2vec(M, R)
    th = M.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    Rr = [n(int(i % 4 == 0)) for i in range(9)] if th < EPS else rodrigues(M, r)
    t = [n(v) for v in t]
    err = np.float32(0)
    for (X, Y), (u, v) in zip(obj, corners):
        pu, pv = project_point(M, n(X), n(Y), Rr, t, cam)
        dx, dy = np.float32(float(pu)) - np.float32(u), np.float32(float(pv)) - np.float32(v)
        err = np.float32(err + np.float32(np.float32(dx * dx) + np.float32(dy * dy)))
    return np.sqrt(np.float32(err / np.float32(8)))


def smallest_eigenvector(a6):
    """the unit eigenvector of the smallest eigenvalue of the symmetric 3 x 3 (a00 a01 a02 a11 a12 a22), by mpmath.eigsy, and the
    relative gap to the next eigenvalue"""
    a00, a01, a02, a11, a12, a22 = [mp.mpf(float(v)) for v in a6]
    E, Q = mp.eigsy(mp.matrix([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]))
    order = sorted(range(3), key=lambda i: E[i])
    v = [Q[i, order[0]] for i in range(3)]
    gap = (E[order[1]] - E[order[0]]) / max(abs(E[order[2]]), mp.mpf(10) ** -300)
    return np.array([float(x) for x in v]), float(gap)


def ho_system(src, dst):
    """the symmetric 3 x 3 of the HO estimator (ippe.cpp:899-1032) for four correspondences, in plain doubles: inputs for the
    eigenvector stage, not a reference of anything"""
    def norm4(p):
        p = np.array(p, np.float64)
        p = p - p.mean(0)
        return p * np.sqrt(8 / (p ** 2).sum())
    a, b = norm4(src), norm4(dst)
    C = np.stack([-b[:, 0] * a[:, 0], -b[:, 0] * a[:, 1], -b[:, 1] * a[:, 0], -b[:, 1] * a[:, 1]], 1)
    C = C - C.mean(0)
    Mx = np.stack([C[:, 0], C[:, 1], -b[:, 0]], 1); My = np.stack([C[:, 2], C[:, 3], -b[:, 1]], 1)
    P = np.linalg.inv(a.T @ a) @ a.T
    D = np.concatenate([Mx - a @ (P @ Mx), My - a @ (P @ My)])
    s = D.T @ D
    return np.array([s[0, 0], s[0, 1], s[0, 2], s[1, 1], s[1, 2], s[2, 2]])


# ------------------------------------------------------------------------------------------------------------------------ the whole solve
def solve(M, corners, size, cam):
    """both IPPE solutions of one marker: {img, H, J, sol: [a, b]} with, per solution, R (9), t (3), rms (exact reprojection RMS of R),
    rvec (the well-conditioned logarithm under MP, rot2vec under F64), w, rad (both radicands)"""
    obj = object_points(size)
    img = [normalise_point(M, u, v, cam) for u, v in corners]
    H = homography(M, obj, img)
    J = jacobian(H)
    R1, R2, rad0, rad1 = rotations(M, J)
    sols = []
    for R in (R1, R2):
        t = translation(M, obj, img, R)
        rvec, w = log_rotation(R) if M is MP else rot2vec(M, R)
        sols.append({"R": R, "t": t, "rms": reprojection_rms(M, obj, corners, cam, R, t), "rvec": rvec, "w": w})
    return {"img": img, "H": H, "J": J, "rad": (rad0, rad1), "sol": sols}


def rounding_change(rvec, R):
    """F: the largest change of an entry of R when its own rotation vector is rounded to float"""
    Rf = rodrigues(MP, [f32(v) for v in rvec])
    return float(max(abs(a - mp.mpf(b)) for a, b in zip(Rf, R)))


def tofloat(v):
    return np.array([float(x) for x in v], np.float64)
