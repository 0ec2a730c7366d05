"""Inputs and plain references of the unit tests of the shared device helpers (tests/test_device_units_gpu.py on the device,
tests/test_device_units_cpu.py for the references and for the conditions these builders promise).  Test infrastructure; numpy,
fractions and math only.  Every builder is seeded and lru_cached: a case is computed once per process and must not be modified."""
import functools
import math
from fractions import Fraction

import numpy as np

cached = functools.lru_cache(maxsize=None)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
RAND_MAX = 2 ** 31 - 1


def bits(a):
    """the array as unsigned words of its item size: equality of these is bit-for-bit equality (-0.0 != +0.0, NaN == the same NaN)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ====================================================================================== A. include/orbfe_math.h
@cached
def atan2_sets():
    """name -> (y, x) float32.  `grid` and `moments` are the domain of the frame path (image moments are integers)."""
    g = np.arange(-255, 256, dtype=np.float32)
    gy, gx = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    rng = np.random.default_rng(20240611)
    m = rng.integers(-3_000_000, 3_000_001, (2, 200_000)).astype(np.float32)
    z = np.array([0.0, -0.0, 1.0, -1.0, 255.0, -255.0], np.float32)
    zy, zx = [a.ravel() for a in np.meshgrid(z, z, indexing="ij")]
    zero = (zy == 0) | (zx == 0)
    s = np.arange(-8, 9, dtype=np.float32)
    sy, sx = [a.ravel() for a in np.meshgrid(s, s, indexing="ij")]
    return {"grid": (gy, gx), "moments": (m[0], m[1]), "signed_zero": (zy[zero], zx[zero]),
            "scaled_2^-100": (sy * np.float32(2.0 ** -100), sx * np.float32(2.0 ** -100)),
            "scaled_2^-140": (sy * np.float32(2.0 ** -140), sx * np.float32(2.0 ** -140))}


def _neighbours(c, k):
    """float32 c with its k neighbours on either side, 2k + 1 columns"""
    cols = {0: c}
    lo = hi = c
    for j in range(1, k + 1):
        lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
        cols[-j], cols[j] = lo, hi
    return np.stack([cols[j] for j in range(-k, k + 1)], 1).ravel()


@cached
def sincos_sets():
    """name -> float32 angles in radians"""
    sweep = np.arange(0, 360, 0.0137, dtype=np.float32) * np.float32(math.pi / 180)
    k = np.arange(-6400, 6401, dtype=np.float64)
    flips = np.concatenate([_neighbours((k * (math.pi / 2)).astype(np.float32), 4), _neighbours(((k + 0.5) * (math.pi / 2)).astype(np.float32), 1)])
    uniform = np.random.default_rng(20240612).uniform(-1e4, 1e4, 300_000).astype(np.float32)
    return {"sweep": sweep, "quadrant_flips": flips, "uniform": uniform}


@cached
def round_sets():
    """name -> float64"""
    k = np.arange(-2 ** 22, 2 ** 22 + 1, 4099, dtype=np.float64) + 0.5
    half = np.stack([np.nextafter(k, -np.inf), k, np.nextafter(k, np.inf)], 1).ravel()
    big = np.array([2.0 ** 30 - 0.5, -(2.0 ** 30 - 0.5)])
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, -2.0 ** -1022, 1e-30, -1e-30])
    return {"halves": half, "big": big, "tiny": tiny}


# TUM1 intrinsics and distortion, as tests/match_batch_cases.py has them (tests/test_device_units_cpu.py checks that they are the same),
# extended to 8 coefficients as tests/test_match_batch_device_gpu.py does and to 12 by small thin-prism terms
TUM1_K = np.array([517.306408, 516.469215, 318.643040, 255.313989], np.float32)
TUM1_DIST = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)
DIST12 = np.concatenate([TUM1_DIST, [0.01, -0.02, 0.005], [1e-3, -5e-4, 2e-4, -1e-4]]).astype(np.float32)
NDIST = (0, 4, 5, 8, 12)


def undistort_k12(ndist):
    """the 12 doubles of orbfe_undistort_point for the first ndist float coefficients"""
    k = np.zeros(12)
    k[:ndist] = DIST12[:ndist].astype(np.float64)
    return k


@cached
def undistort_grid():
    """33 x 25 points over a 640 x 480 frame, from 40 px outside one border to 40 px outside the other"""
    u, v = np.linspace(-40, 679, 33), np.linspace(-40, 519, 25)
    return np.stack([a.ravel() for a in np.meshgrid(u, v, indexing="xy")], 1).astype(np.float32)


# ====================================================================================== B. csrc/wave_dpp.hpp
@cached
def wave_rows_i32(sums):
    """rows of 64 int32: one-hot 1, one-hot -1, the extremes (all INT_MIN, all INT_MAX, alternating either way), 200 random rows.
    sums: the random values stay in +-2^24, so that no order of additions wraps; the sums of the rows of extremes do wrap, which
    is the same in every order (arithmetic modulo 2^32 is associative) and is what numpy's int32 cumsum does too."""
    eye = np.eye(64, dtype=np.int32)
    alt = np.where(np.arange(64) % 2 == 0, INT_MIN, INT_MAX).astype(np.int32)
    rng = np.random.default_rng(20240613)
    rnd = rng.integers(-2 ** 24, 2 ** 24 + 1, (200, 64)) if sums else rng.integers(INT_MIN, INT_MAX + 1, (200, 64))
    return np.concatenate([eye, -eye, np.stack([np.full(64, INT_MIN, np.int32), np.full(64, INT_MAX, np.int32), alt, alt[::-1]]), rnd.astype(np.int32)])


def cumsum16(rows):
    """inclusive scan restarted every 16 lanes"""
    return np.cumsum(rows.reshape(-1, 4, 16), axis=2, dtype=np.int32).reshape(rows.shape)


@cached
def wave_rows_u64():
    """name -> rows of 64 uint64"""
    rng = np.random.default_rng(20240614)
    lo = rng.integers(0, 2 ** 32, (100, 1), dtype=np.uint64)
    hi = rng.integers(0, 2 ** 32, (100, 64), dtype=np.uint64)
    high_only = (hi << np.uint64(32)) | lo                  # equal low words, different high words
    low_only = (lo << np.uint64(32)) | hi                   # the other way round
    base = rng.integers(2 ** 20, 2 ** 63, (64, 64), dtype=np.uint64)
    one_max, one_min = base.copy(), base.copy()
    one_max[np.arange(64), np.arange(64)] = np.uint64(2 ** 64 - 1) - rng.integers(0, 2 ** 10, 64, dtype=np.uint64)
    one_min[np.arange(64), np.arange(64)] = rng.integers(0, 2 ** 10, 64, dtype=np.uint64)
    ends = rng.integers(0, 2 ** 64, (64, 64), dtype=np.uint64)
    ends[np.arange(64), np.arange(64)] = 0
    ends[np.arange(64), (np.arange(64) * 37 + 11) % 64] = np.uint64(2 ** 64 - 1)
    ends = np.concatenate([ends, np.zeros((1, 64), np.uint64), np.full((1, 64), 2 ** 64 - 1, np.uint64)])
    return {"high_word_only": high_only, "low_word_only": low_only, "max_in_lane_i": one_max, "min_in_lane_i": one_min, "zero_and_ones": ends}


@cached
def knn_key_rows():
    """rows of (distance << 32 | position) keys as k_knn2_csr forms them, every row with its smallest distance twice or more; lanes
    without a candidate hold ~0.  Returns (rows, best, second): the keys the oracle's strict '<' scan over the list keeps."""
    rng = np.random.default_rng(20240615)
    rows, best, second = [], [], []
    for r in range(128):
        n = 64 if r < 64 else int(rng.integers(2, 64))
        d = rng.integers(10, 257, n)
        dup = rng.choice(n, 2 + r % 3 if n > 4 else 2, replace=False)
        d[dup] = d.min() - (r % 2)                          # the duplicated minimum: a tie with the old one or below it
        lanes = rng.permutation(64)[:n]                     # which lane holds which list position
        row = np.full(64, 2 ** 64 - 1, np.uint64)
        row[lanes] = (d.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        b_d, b_i, s_d, s_i = 1 << 30, -1, 1 << 30, -1       # the scan in list order: first of equal distances wins
        for i in range(n):
            if d[i] < b_d:
                s_d, s_i, b_d, b_i = b_d, b_i, int(d[i]), i
            elif d[i] < s_d:
                s_d, s_i = int(d[i]), i
        rows.append(row); best.append((b_d << 32) | b_i); second.append((s_d << 32) | s_i)
    return np.stack(rows), np.array(best, np.uint64), np.array(second, np.uint64)


@cached
def wave_rows_f64():
    """name -> rows of 64 doubles whose every partial sum is an integer below 2^53"""
    rng = np.random.default_rng(20240616)
    ints = rng.integers(-2 ** 46, 2 ** 46, (100, 64)).astype(np.float64)    # |sum| < 2^52
    onehot = np.eye(64) * (2.0 ** 52 + 1)
    return {"integers": ints, "one_hot_2^52+1": onehot}


# ====================================================================================== C. csrc/lm_dense.hpp
def quat_to_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


QUAT_AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
QUAT_ANGLES = (10.0, 120.0, 179.9, 180.0)


@cached
def quat_matrices():
    """n x 3 x 3 rotations in float64: QUAT_ANGLES about QUAT_AXES, then the exact half turn about (1,-1,0): m00 == m11 > m22 and trace
    -1, where the strict '>' keeps i = 0 and so x > 0 > y; i = 1 would give the same rotation as -q, which the comparison by
    component tells apart (about (1,1,0) both choices give the same q)"""
    Rs = []
    for ax in QUAT_AXES:
        a = np.array(ax, np.float64) / math.sqrt(sum(c * c for c in ax))
        for deg in QUAT_ANGLES:
            h = math.radians(deg) / 2
            Rs.append(quat_to_matrix(np.concatenate([a * math.sin(h), [math.cos(h)]])))
    Rs.append(np.array([[0., -1, 0], [-1, 0, 0], [0, 0, -1]]))
    return np.stack(Rs)


def quat_branch(m):
    """the branch of Eigen's Quaternion(Matrix3) for m: -1 the trace, else the index of the largest diagonal entry (first of equals)"""
    if m[0, 0] + m[1, 1] + m[2, 2] > 0:
        return -1
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    return i


def quat_ref(m):
    """Eigen's rule in float64, as x y z w"""
    m = np.asarray(m, np.float64)
    i = quat_branch(m)
    if i < 0:
        t = np.sqrt(m[0, 0] + m[1, 1] + m[2, 2] + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t, w])
    j, k = (i + 1) % 3, (i + 2) % 3
    v = np.zeros(4)
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    v[i] = 0.5 * t
    t = 0.5 / t
    v[3] = (m[k, j] - m[j, k]) * t
    v[j] = (m[j, i] + m[i, j]) * t
    v[k] = (m[k, i] + m[i, k]) * t
    return v


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def rotate_ref(q, v):
    """lm_dense.hpp's rotate in its operation order: uv = 2 (qv x v), r = (v + w uv) + qv x uv"""
    uv = _cross(q[:, :3], v)
    uv = uv + uv
    return (v + q[:, 3:4] * uv) + _cross(q[:, :3], uv)


def qmul_ref(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], 1)


def project_ref(Xc, obs, cam, info):
    fx, fy, cx, cy = cam
    e = np.stack([obs[:, 0] - ((Xc[:, 0] / Xc[:, 2]) * fx + cx), obs[:, 1] - ((Xc[:, 1] / Xc[:, 2]) * fy + cy)], 1)
    return e, e[:, 0] * (info * e[:, 0]) + e[:, 1] * (info * e[:, 1])


@cached
def dense_inputs():
    """random unit-ish quaternions, vectors, camera points and observations (float64) for rotate / qmul / project_error / chi2_of"""
    rng = np.random.default_rng(20240617)
    n = 1000
    qa, qb = rng.normal(size=(n, 4)), rng.normal(size=(n, 4))
    qa /= np.linalg.norm(qa, axis=1, keepdims=True)
    Xc = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(0.3, 12, (n, 1))], 1)
    cam = TUM1_K.astype(np.float64)
    obs = np.stack([Xc[:, 0] / Xc[:, 2] * cam[0] + cam[2], Xc[:, 1] / Xc[:, 2] * cam[1] + cam[3]], 1) + rng.normal(0, 2, (n, 2))
    return dict(qa=qa, qb=qb, v=rng.uniform(-10, 10, (n, 3)), Xc=Xc, obs=obs, cam=cam, info=1.0 / 1.2 ** (2 * rng.integers(0, 8, n)))


def huber_linear(chi2, delta):
    """the branch of chi2 > delta^2, in the header's operation order"""
    s = np.sqrt(np.float64(chi2))
    return 2 * s * delta - delta * delta, delta / s


HUBER_DELTAS = (math.sqrt(5.991), math.sqrt(7.815))


@cached
def huber_inputs():
    """(chi2, delta, expects_quadratic): below, at and above delta * delta for the two deltas of the optimizers.  At chi2 == delta^2
    the linear branch gives the quadratic branch's bits (sqrt(delta * delta) == delta in double, tests/test_device_units_cpu.py), so the
    equality case is held to the quadratic values; one ulp above, the linear formula is what is compared."""
    chi2, delta, quad = [], [], []
    for d in HUBER_DELTAS:
        dsqr = d * d
        for c, q in ((0.0, True), (1e-3, True), (0.5 * dsqr, True), (np.nextafter(dsqr, 0), True), (dsqr, True),
                     (np.nextafter(dsqr, np.inf), False), (1.5 * dsqr, False), (10.0, False), (1e4, False), (1e12, False)):
            chi2.append(c); delta.append(d); quad.append(q)
    return np.array(chi2), np.array(delta), np.array(quad)


def huber_ref(chi2, delta):
    dsqr = delta * delta
    s = np.sqrt(chi2)
    with np.errstate(divide="ignore"):
        return np.where(chi2 <= dsqr, chi2, 2 * s * delta - dsqr), np.where(chi2 <= dsqr, 1.0, delta / s)


# ---- ldlt_solve: H = P L D L^T P^T in exact dyadic rationals
LDLT_CLASSES = {"a": 80, "b": 30, "c": 20, "d": 2, "e": 38, "f": 30}     # 200 systems per N
LDLT_D = (Fraction(1, 4), Fraction(1, 2), Fraction(1), Fraction(2), Fraction(4), Fraction(8))
KAPPA_MAX = 1e6
SENTINEL = -12345.678


def _frac_matrix(rows):
    return [[Fraction(v) for v in r] for r in rows]


def frac_inverse(A):
    """exact inverse by Gauss-Jordan elimination; None when singular"""
    n = len(A)
    M = [list(r) + [Fraction(int(i == j)) for j in range(n)] for i, r in enumerate(A)]
    for c in range(n):
        p = next((r for r in range(c, n) if M[r][c] != 0), None)
        if p is None:
            return None
        M[c], M[p] = M[p], M[c]
        piv = M[c][c]
        M[c] = [v / piv for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [r[n:] for r in M]


def frac_pivots(A):
    """the pivots of the exact LDLT with diagonal pivoting on the largest remaining |diagonal| (first of equals), and the first
    pivot's position; None when a pivot is zero"""
    A = [list(r) for r in A]
    n = len(A)
    piv, first = [], None
    for k in range(n):
        big = max(range(k, n), key=lambda i: (abs(A[i][i]), -i))
        if k == 0:
            first = big
        if A[big][big] == 0:
            return None, first
        A[k], A[big] = A[big], A[k]
        for r in A:
            r[k], r[big] = r[big], r[k]
        piv.append(A[k][k])
        for i in range(k + 1, n):
            f = A[i][k] / A[k][k]
            A[i] = [a - f * b for a, b in zip(A[i], A[k])]
    return piv, first


def _ldl_matrix(rng, n, signs, identity_perm):
    L = [[Fraction(int(i == j)) if j >= i else Fraction(int(rng.integers(-8, 9)), 8) for j in range(n)] for i in range(n)]
    d = [LDLT_D[int(rng.integers(0, len(LDLT_D)))] * s for s in signs]
    perm = list(range(n)) if identity_perm else [int(v) for v in rng.permutation(n)]
    A = [[sum(L[i][k] * d[k] * L[j][k] for k in range(n)) for j in range(n)] for i in range(n)]
    return [[A[perm[i]][perm[j]] for j in range(n)] for i in range(n)]


def _inf_norm(A):
    return max(sum(abs(v) for v in r) for r in A)


def _system(cls, H, b, expect_ok, keep=None):
    """one case: floats for the device, the exact solution rounded to double, kappa_inf from the exact inverse (over the rows and
    columns `keep`, the non-zero block of class e; everything otherwise)"""
    n = len(H)
    keep = list(range(n)) if keep is None else keep
    x, kappa = [Fraction(0)] * n, 0.0
    if keep and expect_ok:
        Hs = [[H[i][j] for j in keep] for i in keep]
        inv = frac_inverse(Hs)
        kappa = float(_inf_norm(Hs) * _inf_norm(inv))
        for a, i in enumerate(keep):
            x[i] = sum(inv[a][c] * b[j] for c, j in enumerate(keep))
    Hf = np.array([[float(v) for v in r] for r in H])
    assert all(Fraction(v) == w for r, rw in zip(Hf, H) for v, w in zip(r, rw)), "H is not an exact double"
    return dict(cls=cls, H=Hf, b=np.array([float(v) for v in b]), x=np.array([float(v) for v in x]), ok=expect_ok, kappa=kappa,
                keep=np.array(keep, np.int64), first_pivot=frac_pivots(H)[1])


@cached
def ldlt_systems(N):
    """200 systems of size N over the classes of LDLT_CLASSES; see tests/test_device_units_gpu.py::test_ldlt_solve"""
    rng = np.random.default_rng(20240618 + N)
    out = []

    def rhs(n=N):
        b = [Fraction(int(rng.integers(-32, 33)), 8) for _ in range(n)]
        return b if any(b) else rhs(n)

    def full(cls, signs_of, ok):
        for c in range(LDLT_CLASSES[cls]):
            while True:
                H = _ldl_matrix(rng, N, signs_of(), identity_perm=(c == 0))
                inv = frac_inverse(H)
                if frac_pivots(H)[0] is not None and float(_inf_norm(H) * _inf_norm(inv)) <= KAPPA_MAX:
                    break
            out.append(_system(cls, H, rhs(), ok))

    full("a", lambda: [1] * N, True)
    full("b", lambda: [-1 if i == j else 1 for j in [int(rng.integers(0, N))] for i in range(N)], False)
    full("c", lambda: [-1] * N, False)
    for _ in range(LDLT_CLASSES["d"]):
        out.append(_system("d", [[Fraction(0)] * N for _ in range(N)], rhs(), True, keep=[]))
    for c in range(LDLT_CLASSES["e"]):
        while True:
            B = _ldl_matrix(rng, 5, [1] * 5, identity_perm=(c == 0))
            if float(_inf_norm(B) * _inf_norm(frac_inverse(B))) <= KAPPA_MAX:
                break
        keep = sorted(int(v) for v in rng.permutation(N)[:5])
        H = [[Fraction(0)] * N for _ in range(N)]
        for a, i in enumerate(keep):
            for c2, j in enumerate(keep):
                H[i][j] = B[a][c2]
        b = rhs()
        while any(b[i] == 0 for i in range(N) if i not in keep):
            b = rhs()
        out.append(_system("e", H, b, True, keep=keep))
    for c in range(LDLT_CLASSES["f"]):
        d = [Fraction(2) ** (N - 1 - i - 3) for i in range(N)]               # 2^(N-4) .. 1/8, descending
        d = d if c == 0 else d[::-1] if c == 1 else [d[int(i)] for i in rng.permutation(N)]
        out.append(_system("f", [[d[i] if i == j else Fraction(0) for j in range(N)] for i in range(N)], rhs(), True))
    return out


def ldlt_ratio(case, x):
    """r = |x - x*|_inf / (eps kappa_inf |x*|_inf) over the case's non-zero block"""
    k = case["keep"]
    return float(np.max(np.abs(x[k] - case["x"][k])) / (np.finfo(np.float64).eps * case["kappa"] * np.max(np.abs(case["x"][k]))))


@cached
def ldlt_numpy_worst(N):
    """the worst ratio of numpy.linalg.solve (LAPACK's partial-pivoting LU) over the solvable systems of ldlt_systems(N)"""
    worst = 0.0
    for c in ldlt_systems(N):
        if c["ok"] and len(c["keep"]):
            k = c["keep"]
            x = np.zeros(N)
            x[k] = np.linalg.solve(c["H"][np.ix_(k, k)], c["b"][k])
            worst = max(worst, ldlt_ratio(c, x))
    return worst


# ---- block_sum: the documented order
def block_sum_ref(v):
    """v: 256 x N doubles -> N sums: the xor butterfly 32, 16 .. 1 inside each wave of 64, then waves 0 .. 3 in order"""
    w = np.array(v, np.float64).reshape(4, 64, -1)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ off]
    s = w[0, 0]
    for ww in range(1, 4):
        s = s + w[ww, 0]
    return s


def left_to_right(v):
    s = np.zeros(v.shape[1])
    for row in np.asarray(v, np.float64):
        s = s + row
    return s


@cached
def block_sum_inputs(N):
    """nblk x 256 x N doubles with magnitudes spread over 2^0 .. 2^60 and mixed signs, so that the order of the additions shows"""
    rng = np.random.default_rng(20240619 + N)
    shape = (6, 256, N)
    return rng.uniform(1, 2, shape) * 2.0 ** rng.integers(0, 61, shape) * rng.choice([-1.0, 1.0], shape)


BLOCK_COUNT_AT = (0, 63, 64, 255)


@cached
def block_count_inputs():
    """rows of 256 flags with totals 0, 1 (at BLOCK_COUNT_AT), 255 (all but BLOCK_COUNT_AT) and 256"""
    rows = [np.zeros(256, np.int32)]
    for t in BLOCK_COUNT_AT:
        one = np.zeros(256, np.int32); one[t] = 1
        rows += [one, 1 - one]
    rows.append(np.ones(256, np.int32))
    return np.stack(rows)


# ====================================================================================== D. csrc/ransac_sets.hpp
SET_N = (None, None, 9, 10, 16, 100, 2000)       # None: K and K + 1
SETS_PER_FAMILY = 600                            # five families: 3000 sets per (K, N)
SETS_OUT_OF_RANGE = 200


def set_sizes(K):
    return tuple(dict.fromkeys([K, K + 1] + [n for n in SET_N if n is not None]))


def clamp_word(w, size):
    """RandomInt(0, size - 1) on the rand() word w as the reference computes it, then the header's clamp for words outside 0 .. RAND_MAX"""
    r = int((float(w) / (2147483647.0 + 1.0)) * size)      # int(): towards zero, as the C++ cast
    return 0 if r < 0 else size - 1 if r >= size else r


def draw_ref(words, N):
    """the reference's draw (Initializer.cc:80-97, Sim3Solver.cc:163-177): the list of available indices, take the entry, overwrite it
    with the last, pop"""
    avail = list(range(N))
    out = []
    for w in words:
        r = clamp_word(int(w), len(avail))
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def draw_sparse(words, N):
    """a transcription of decode_set's sparse form: only the positions of the list that differ from the identity are kept"""
    pos, val, out = [], [], []
    for j, w in enumerate(words):
        size = N - j
        r = clamp_word(int(w), size)
        idx, back = r, size - 1
        for p, v in zip(pos, val):
            if p == r:
                idx = v
        for p, v in zip(pos, val):
            if p == size - 1:
                back = v
        out.append(idx)
        if r in pos:
            val[pos.index(r)] = back
        else:
            pos.append(r); val.append(back)
    return out


@cached
def set_words(K, N):
    """name -> sets x K int32 words.  The first five families are rand() words (0 .. RAND_MAX); `out_of_range` mixes in -1, INT_MIN
    and other words a rand() cannot return, which decode_set documents and clamps."""
    rng = np.random.default_rng(20240620 + 131 * K + N)
    n = SETS_PER_FAMILY
    rep = rng.integers(0, 2 ** 31, (n, 1))
    fam = {"random": rng.integers(0, 2 ** 31, (n, K)), "all_zero": np.zeros((n, K)), "all_rand_max": np.full((n, K), RAND_MAX),
           "three_values": rng.choice([0, 2 ** 30, RAND_MAX], (n, K)), "one_word_repeated": np.repeat(rep, K, 1)}
    bad = rng.integers(0, 2 ** 31, (SETS_OUT_OF_RANGE, K))
    hit = rng.random(bad.shape) < 0.5
    bad[hit] = rng.choice([-1, INT_MIN, -2 ** 30, INT_MIN + 1], int(hit.sum()))
    bad[0], bad[1] = -1, INT_MIN
    fam["out_of_range"] = bad
    return {k: v.astype(np.int32) for k, v in fam.items()}


@cached
def set_expected(K, N):
    return {name: np.array([draw_ref(row, N) for row in w], np.int32) for name, w in set_words(K, N).items()}


CLAMP_CAPS = (0, 1, 7, 2000, INT_MAX)


@cached
def clampn_inputs():
    n, cap = [], []
    for c in CLAMP_CAPS:
        for v in (-1, 0, c, min(c + 1, INT_MAX), INT_MIN, INT_MAX, c // 2):
            n.append(v); cap.append(c)
    return np.array(n, np.int32), np.array(cap, np.int32)


# ====================================================================================== E. csrc/sim3_points.hpp
@cached
def rigid_inputs():
    """1000 poses [R | t] (float32, rotations to float precision) and points"""
    rng = np.random.default_rng(20240621)
    n = 1000
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    T = np.concatenate([np.stack([quat_to_matrix(v) for v in q]), rng.uniform(-5, 5, (n, 3, 1))], 2).astype(np.float32)
    return T.reshape(n, 12), rng.uniform(-20, 20, (n, 3)).astype(np.float32)


def rigid_ref(T, p):
    """float inputs, double products summed in index order, plus the translation, rounded once"""
    T, p = T.astype(np.float64).reshape(-1, 3, 4), p.astype(np.float64)
    return (((T[:, :, 0] * p[:, 0:1] + T[:, :, 1] * p[:, 1:2]) + T[:, :, 2] * p[:, 2:3]) + T[:, :, 3]).astype(np.float32)


def rigid_float_only(T, p):
    T = T.reshape(-1, 3, 4)
    return ((T[:, :, 0] * p[:, 0:1] + T[:, :, 1] * p[:, 1:2]) + T[:, :, 2] * p[:, 2:3]) + T[:, :, 3]
