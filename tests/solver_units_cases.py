"""Inputs and references of the unit tests of the optimizers' and solvers' device helpers (tests/test_solver_units_gpu.py on the device,
tests/test_solver_units_cpu.py for the references and for the conditions these builders promise).  Test infrastructure; numpy, math,
fractions and mpmath only.  Every builder is seeded and lru_cached: a case is computed once per process and must not be modified.

Three kinds of reference stand here:
  plain   the helper's operations in its own order on IEEE doubles (Python floats or numpy, which never contract), for bit equality;
          next to each a differently ordered evaluation that gives other bits, so that equality says something
  closed  g2o's closed forms (the branches taken as the header takes them, decided in double) evaluated with mpmath at 50 digits:
          what the device's and the restatement's rounding errors are measured against
  true    the definition (the matrix exponential, the derivative), which a misreading shared by kernel and restatement would miss"""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

import device_units_cases as K

cached = functools.lru_cache(maxsize=None)
bits = K.bits
EPS = float(np.finfo(np.float64).eps)
FEPS = float(np.finfo(np.float32).eps)
MP = mpmath.mp.clone()
MP.dps = 50
NCLASS = 200          # inputs a class where an error is measured: the worst of 200 on two libms are comparable
# The floors of BOUND = max(4 x the host restatement's worst error, floor).  SE3Quat's is given with the tests' design; Sim3's
# constructor is the same closed forms; Sim3::log applies acos and a 3 x 3 solve to what such forms gave, two such steps in a row.
SE3_FLOOR, SIM3_FLOOR, SIM3_LOG_FLOOR = 16.0, 16.0, 32.0
THRESH = 0.00001      # g2o's eps of the exponential maps


class _F:
    """double arithmetic for the closed forms: Python floats round every operation once, in the written order"""
    sqrt, sin, cos, exp, log, acos = math.sqrt, math.sin, math.cos, math.exp, math.log, math.acos
    one = 1.0

    @staticmethod
    def num(v):
        return float(v)


class _M:
    sqrt, sin, cos, exp, log, acos = MP.sqrt, MP.sin, MP.cos, MP.exp, MP.log, MP.acos
    one = MP.mpf(1)

    @staticmethod
    def num(v):
        return MP.mpf(float(v))


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))


def rows_differing(a, b):
    """the fraction of rows (first axis) on which a and b differ in any bit"""
    a, b = bits(np.asarray(a)).reshape(len(a), -1), bits(np.asarray(b)).reshape(len(b), -1)
    return float((a != b).any(1).mean())


# ====================================================================================== shared closed forms (F = _F or _M)
def _skew(w):
    return [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]


def _matmul3(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def _quat_of(m, F):
    """Eigen's Quaternion(Matrix3) as x y z w"""
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        t = F.sqrt(t + 1)
        w = t / 2
        t = (F.one / 2) / t
        return [(m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t, w]
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    v = [0, 0, 0, 0]
    t = F.sqrt(m[i][i] - m[j][j] - m[k][k] + 1)
    v[i] = t / 2
    t = (F.one / 2) / t
    v[3] = (m[k][j] - m[j][k]) * t
    v[j] = (m[j][i] + m[i][j]) * t
    v[k] = (m[k][i] + m[i][k]) * t
    return v


def _normalized(q, F, reciprocal=False):
    if q[3] < 0:
        q = [-c for c in q]
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if n2 > 0:
        n = F.sqrt(n2)
        q = [c * (1 / n) for c in q] if reciprocal else [c / n for c in q]
    return q


def _rot_matrix(q):
    """Eigen's toRotationMatrix of x y z w, not normalised"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def theta_of(u):
    """the angle as the headers compute it: the sum of squares in order, then sqrt, in double"""
    return math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])


def se3_exp_form(u, small, F=_F, variant=False):
    """SE3Quat::exp's closed form of the given branch as q (x y z w), t; variant: the differently ordered evaluation (the translation's
    three products summed from the right, the quaternion times 1 / n instead of divided by n)"""
    u = [F.num(c) for c in u]
    om = u[:3]
    theta = F.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    O = _skew(om)
    O2 = _matmul3(O, O)
    I = [[1 if i == j else 0 for j in range(3)] for i in range(3)]
    if small:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        a, b = F.sin(theta) / theta, (1 - F.cos(theta)) / (theta * theta)
        c = (theta - F.sin(theta)) / (theta * theta * theta)
        R = [[(I[i][j] + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
        V = [[(I[i][j] + b * O[i][j]) + c * O2[i][j] for j in range(3)] for i in range(3)]
    if variant:
        t = [V[i][2] * u[5] + V[i][1] * u[4] + V[i][0] * u[3] for i in range(3)]
    else:
        t = [V[i][0] * u[3] + V[i][1] * u[4] + V[i][2] * u[5] for i in range(3)]
    return _normalized(_quat_of(R, F), F, variant) + t


def _abc(sigma, s, theta, small_s, small_t, F):
    if small_s:
        C = F.one
        if small_t:
            A, B = F.one / 2, F.one / 6
        else:
            t2 = theta * theta
            A, B = (1 - F.cos(theta)) / t2, (theta - F.sin(theta)) / (t2 * theta)
    else:
        C = (s - 1) / sigma
        if small_t:
            s2 = sigma * sigma
            A, B = ((sigma - 1) * s + 1) / s2, ((s2 / 2 - sigma + 1) * s) / (s2 * sigma)
        else:
            a, b = s * F.sin(theta), s * F.cos(theta)
            t2, s2 = theta * theta, sigma * sigma
            c = t2 + s2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1 / t2
    return A, B, C


def sim3_exp_form(u, small_t, small_s, F=_F):
    """Sim3(Vector7d)'s closed form of the given branches as q (x y z w, as it is), t, s"""
    u = [F.num(c) for c in u]
    om, sigma = u[:3], u[6]
    theta = F.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    O = _skew(om)
    O2 = _matmul3(O, O)
    I = [[1 if i == j else 0 for j in range(3)] for i in range(3)]
    s = F.exp(sigma)
    if small_t:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
    else:
        a, b = F.sin(theta) / theta, (1 - F.cos(theta)) / (theta * theta)
        R = [[(I[i][j] + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
    A, B, C = _abc(sigma, s, theta, small_s, small_t, F)
    W = [[(A * O[i][j] + B * O2[i][j]) + C * I[i][j] for j in range(3)] for i in range(3)]
    t = [W[i][0] * u[3] + W[i][1] * u[4] + W[i][2] * u[5] for i in range(3)]
    return _quat_of(R, F) + t + [s]


def log_d(S):
    """d of Sim3::log as the header computes it, in double"""
    R = _rot_matrix([float(c) for c in S[:4]])
    return 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)


def log_branches(S):
    """(|sigma| < 1e-5, d > 1 - 1e-5) as the header decides them, in double"""
    return abs(math.log(float(S[7]))) < THRESH, log_d(S) > 1 - THRESH


def sim3_log_form(S, small_s, small_d, F=_M):
    """Sim3::log's closed form of the given branches: omega, upsilon, sigma (the 3 x 3 solve exactly enough: mpmath's lu_solve)"""
    S = [F.num(c) for c in S]
    R = _rot_matrix(S[:4])
    s = S[7]
    sigma = F.log(s)
    d = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    theta = 0
    if small_d:
        om = [c / 2 for c in dR]
    else:
        theta = F.acos(d)
        f = theta / (2 * F.sqrt(1 - d * d))
        om = [f * c for c in dR]
    A, B, C = _abc(sigma, s, theta, small_s, small_d, F)
    O = _skew(om)
    O2 = _matmul3(O, O)
    W = MP.matrix([[(A * O[i][j] + B * O2[i][j]) + C * (1 if i == j else 0) for j in range(3)] for i in range(3)])
    ups = MP.lu_solve(W, MP.matrix(S[4:7]))
    return om + [ups[i] for i in range(3)] + [sigma]


def as_float(v):
    return np.array([float(c) for c in v])


def err_units(got, want_mp, unit):
    """max |got - want| / unit with the difference taken at 50 digits"""
    return max(float(abs(MP.mpf(float(g)) - w)) for g, w in zip(np.asarray(got).ravel(), want_mp)) / unit


# ---- true: matrices and the matrix exponential
def generator(u):
    """the 4 x 4 generator of omega, upsilon (and sigma when u has 7)"""
    u = [MP.mpf(float(c)) for c in u]
    G = MP.zeros(4)
    O = _skew(u[:3])
    for i in range(3):
        for j in range(3):
            G[i, j] = O[i][j] + (u[6] if len(u) == 7 and i == j else 0)
        G[i, 3] = u[3 + i]
    return G


def expm_series(G):
    """the matrix exponential by scaling and squaring of its Taylor series at 50 digits: the second route next to mpmath.expm"""
    k = max(0, int(math.ceil(math.log2(max(float(MP.mnorm(G, 1)), 1e-300)))) + 8)
    A = G / MP.mpf(2) ** k
    out, term = MP.eye(4), MP.eye(4)
    for i in range(1, 40):
        term = term * A / i
        out = out + term
    for _ in range(k):
        out = out * out
    return out


def matrix_of(T):
    """[s R t; 0 1] of q (x y z w, as it is), t and, when T has 8, s; at 50 digits"""
    T = [MP.mpf(float(c)) for c in T]
    R = _rot_matrix(T[:4])
    s = T[7] if len(T) == 8 else 1
    M = MP.eye(4)
    for i in range(3):
        for j in range(3):
            M[i, j] = s * R[i][j]
        M[i, 3] = T[4 + i]
    return M


def max_abs(M):
    return max(float(abs(c)) for c in M)


# ====================================================================================== A. csrc/se3_quat.hpp
def _directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


@cached
def se3_exp_inputs():
    """class -> n x 6 (omega, upsilon).  tiny, cancel and large are NCLASS each; threshold: theta at 1e-5 and its two neighbours along
    each axis and along a diagonal (nine and three inputs)"""
    rng = np.random.default_rng(2001)
    out = {}
    for name, lo, hi in (("tiny", 1e-9, 0.99e-5), ("cancel", 1.01e-5, 1e-3), ("large", 1e-3, 3.1)):
        out[name] = np.concatenate([_directions(rng, NCLASS) * _log_uniform(rng, lo, hi, NCLASS)[:, None], rng.uniform(-5, 5, (NCLASS, 3))], 1)
    out["zero"] = np.concatenate([np.zeros((NCLASS, 3)), rng.uniform(-5, 5, (NCLASS, 3))], 1)
    out["zero"][0] = 0
    th = []
    for t in (np.nextafter(THRESH, 0), THRESH, np.nextafter(THRESH, 1)):
        for ax in range(3):
            w = np.zeros(3)
            w[ax] = t
            th.append(np.concatenate([w, [0.4, -1.1, 0.8]]))
        th.append(np.concatenate([np.array([2., -1, 2]) / 3 * t, [0.4, -1.1, 0.8]]))
    out["threshold"] = np.array(th)
    return out


def se3_small(u):
    return theta_of(u) < THRESH


def se3_exp_unit(u):
    return EPS * max(1.0, float(np.abs(u).max()))


@cached
def se3_exp_closed(name):
    """the closed form of the branch the header takes, at 50 digits, for every input of the class"""
    return [se3_exp_form(u, se3_small(u), _M) for u in se3_exp_inputs()[name]]


def se3_exp_worst(name, got):
    return max(err_units(g, w, se3_exp_unit(u)) for u, g, w in zip(se3_exp_inputs()[name], got, se3_exp_closed(name)))


def se3_truth_tolerance(u):
    """test_essential_cpu's formula: 1e3 eps, over the divisor theta of the closed forms where it is small (as its tol_log has it),
    and g2o's own truncation in the small branch: theta^2 on R, and theta |upsilon| on t, since V = R = I + Omega + Omega^2 there
    where the series has Omega / 2"""
    theta = theta_of(u)
    small = theta < THRESH
    tol = 1e3 * EPS / (1.0 if small else min(1.0, theta)) + (theta ** 2 + theta * float(np.linalg.norm(u[3:6])) if small else 0)
    return 4 * tol * max(1.0, float(np.abs(u).max()))


@cached
def normalize_inputs():
    """random quaternions of both signs of w and scales 2^-8 .. 2^8, then the edges: w == -0.0 (not negative: the vector part keeps
    its sign), a zero quaternion (left as it is), norm 2^-540 (n2 underflows to 0: left as it is) and w < 0 of that norm (negated only)"""
    rng = np.random.default_rng(2002)
    q = rng.normal(size=(NCLASS, 4)) * 2.0 ** rng.integers(-8, 9, (NCLASS, 1))
    tiny = np.array([0.5, -0.5, 0.5, 0.5]) * 2.0 ** -540
    edges = np.array([[0.6, -0.8, 0.0, -0.0], [0.0, 0.0, 0.0, 0.0], [-0.0, 0.0, -0.0, -0.0], tiny, -tiny, [0, 0, 0, -3.0], [1, 2, 3, 0.0]])
    return np.concatenate([q, edges])


def normalize_reciprocal(q):
    """the differently ordered evaluation: times 1 / n instead of divided by n"""
    q = np.where(q[:, 3:4] < 0, -q, q)
    n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    with np.errstate(all="ignore"):
        inv = 1.0 / np.sqrt(n2)
        return np.where((n2 > 0)[:, None], q * inv[:, None], q)


def random_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


@cached
def se3_pairs():
    """(a, b, p): NCLASS pairs of SE3 (unit quaternions to double rounding, some with w < 0 so that the product's normalisation flips)
    and points"""
    rng = np.random.default_rng(2003)
    a = np.concatenate([random_quats(rng, NCLASS), rng.uniform(-5, 5, (NCLASS, 3))], 1)
    b = np.concatenate([random_quats(rng, NCLASS), rng.uniform(-5, 5, (NCLASS, 3))], 1)
    return a, b, rng.uniform(-10, 10, (NCLASS, 3))


def rotate_by_matrix(q, v):
    """the differently ordered evaluation of q v: through the rotation matrix of q"""
    return np.stack([np.array(_rot_matrix(list(qq))) @ vv for qq, vv in zip(q, v)])


def se3_map_by_matrix(a, p):
    return rotate_by_matrix(a[:, :4], p) + a[:, 4:]


def se3_mul_by_matrix(a, b):
    """q as the header's (through the restatement's bits is the test's business); t through the matrix: columns 4..6 only"""
    return a[:, 4:] + rotate_by_matrix(a[:, :4], b[:, 4:])


def qmul_paired(a, b):
    """the differently ordered evaluation of the quaternion product: the four products of a component summed two and two"""
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([(aw * bx + ax * bw) + (ay * bz - az * by), (aw * by + ay * bw) + (az * bx - ax * bz), (aw * bz + az * bw) + (ax * by - ay * bx),
                     (aw * bw - ax * bx) - (ay * by + az * bz)], 1)


def normalize_plain(q):
    """normalize_rotation on doubles in the header's order (numpy)"""
    q = np.where(q[:, 3:4] < 0, q * -1, q)
    n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    with np.errstate(all="ignore"):
        return np.where((n2 > 0)[:, None], q / np.sqrt(n2)[:, None], q)


@cached
def float_poses():
    """n x 12 float: the rotations of K.quat_matrices() (every branch of quat_from_matrix) rounded to float, with translations"""
    rng = np.random.default_rng(2004)
    R = K.quat_matrices()
    Rt = np.concatenate([R, rng.uniform(-5, 5, (len(R), 3, 1))], 2)
    return Rt.astype(np.float32).reshape(-1, 12)


# ====================================================================================== B. csrc/sim3_group.hpp
SIM3_EXP_CLASSES = {"small_small": (True, True), "large_theta": (False, True), "large_sigma": (True, False), "large_large": (False, False)}


@cached
def sim3_exp_inputs():
    """class -> n x 7 (omega, upsilon, sigma).  The four branch combinations, NCLASS each: theta in [1e-9, 1e-5) or [1e-2, 3.0],
    |sigma| in [1e-9, 1e-5) or [0.05, 1] -- away from theta in [1e-5, 1e-2] and from |sigma| just above 1e-5, where the closed forms
    divide a difference that cancels by theta^2 or sigma^2 and the error is the libm's last bit times 1 / theta; those ranges are in
    theta_threshold and sigma_threshold (1e-5 and its neighbours, with the other argument large), measured as classes of their own."""
    rng = np.random.default_rng(2101)
    out = {}
    for name, (small_t, small_s) in SIM3_EXP_CLASSES.items():
        theta = _log_uniform(rng, 1e-9, 0.99e-5, NCLASS) if small_t else _log_uniform(rng, 1e-2, 3.0, NCLASS)
        sigma = (_log_uniform(rng, 1e-9, 0.99e-5, NCLASS) if small_s else rng.uniform(0.05, 1, NCLASS)) * rng.choice([-1., 1.], NCLASS)
        out[name] = np.concatenate([_directions(rng, NCLASS) * theta[:, None], rng.uniform(-5, 5, (NCLASS, 3)), sigma[:, None]], 1)
    near = (np.nextafter(THRESH, 0), THRESH, np.nextafter(THRESH, 1))
    out["theta_threshold"] = np.array([np.concatenate([np.roll([t, 0, 0], ax), [0.4, -1.1, 0.8], [s]]) for t in near for ax in range(3) for s in (0.25, 3e-6)])
    out["sigma_threshold"] = np.array([np.concatenate([np.array([0.6, -0.3, 0.74]) * th, [0.4, -1.1, 0.8], [sg * s]])
                                       for s in near for sg in (-1, 1) for th in (0.7, 2e-6)])
    return out


def sim3_exp_branches(u):
    return theta_of(u) < THRESH, abs(u[6]) < THRESH


def sim3_unit(u):
    return EPS * max(1.0, float(np.abs(u).max()))


@cached
def sim3_exp_closed(name):
    return [sim3_exp_form(u, *sim3_exp_branches(u), _M) for u in sim3_exp_inputs()[name]]


def sim3_exp_worst(name, got):
    return max(err_units(g, w, sim3_unit(u)) for u, g, w in zip(sim3_exp_inputs()[name], got, sim3_exp_closed(name)))


def sim3_truth_tolerance(u):
    """test_exp_and_log_against_the_matrix_exponential's formula, its 1e3 eps over the divisor of the closed forms that is small (theta
    of A, sigma of C in their large branches), as that test's docstring and its tol_log have it"""
    theta, sigma, up = theta_of(u), abs(u[6]), float(np.linalg.norm(u[3:6]))
    small_t, small_s = theta < THRESH, sigma < THRESH
    tol = 1e3 * EPS / min(1.0, 1.0 if small_t else theta, 1.0 if small_s else sigma) + (theta ** 2 if small_t else 0) + (sigma if small_s else 0) * 2
    if small_t and not small_s:
        tol += theta ** 2 * up / sigma ** 3
    return tol * 4 * max(1.0, float(np.abs(u).max()))


def sim3_tol_log(u):
    """the round trips' tolerance of the same test"""
    theta, sigma, up = theta_of(u), abs(u[6]), float(np.linalg.norm(u[3:6]))
    tol = 1e3 * EPS / min(1.0, theta) + (theta ** 2 if theta < 4.5e-3 else 0) * 4 + (sigma * 2 if sigma < THRESH else 0)
    if theta < 4.5e-3 and sigma >= THRESH:
        tol += theta ** 2 * up / sigma ** 3 * 2
    return tol * max(1.0, float(np.abs(u).max()))


SIM3_LOG_CLASSES = {"small_small": (True, True), "large_d": (True, False), "log_small_d": (False, True), "large_large": (False, False)}


@cached
def sim3_log_sources():
    """class -> n x 7, what the inputs of log are the exponentials of.  (|sigma| < 1e-5, d > 1 - 1e-5): small_small has theta < 1e-5, so
    its quaternions are the not normalised ones of exp's small branch; log_small_d is test_essential_cpu's case, theta in [1e-4, 4e-3]
    (above exp's threshold, below log's, which is on the cosine) with |sigma| in [0.05, 1]; the others have theta in [1e-2, 3.0]."""
    rng = np.random.default_rng(2102)
    out = {}
    for name, (small_s, small_d) in SIM3_LOG_CLASSES.items():
        if name == "small_small":
            theta = _log_uniform(rng, 1e-9, 0.99e-5, NCLASS)
        elif name == "log_small_d":
            theta = _log_uniform(rng, 1e-4, 4e-3, NCLASS)
        else:
            theta = _log_uniform(rng, 1e-2, 3.0, NCLASS)
        sigma = (_log_uniform(rng, 1e-9, 0.99e-5, NCLASS) if small_s else rng.uniform(0.05, 1, NCLASS)) * rng.choice([-1., 1.], NCLASS)
        out[name] = np.concatenate([_directions(rng, NCLASS) * theta[:, None], rng.uniform(-5, 5, (NCLASS, 3)), sigma[:, None]], 1)
    return out


def sim3_mul_plain(a, b):
    """g2o::Sim3's product on doubles in the header's order (numpy)"""
    q = K.qmul_ref(a[:, :4], b[:, :4])
    t = a[:, 7:8] * K.rotate_ref(a[:, :4], b[:, 4:7]) + a[:, 4:7]
    return np.concatenate([q, t, (a[:, 7] * b[:, 7])[:, None]], 1)


def sim3_inverse_plain(a):
    q = a[:, :4] * np.array([-1., -1, -1, 1])
    c = -1.0 / a[:, 7:8]
    return np.concatenate([q, K.rotate_ref(q, c * a[:, 4:7]), 1.0 / a[:, 7:8]], 1)


def sim3_inverse_by_matrix(a):
    """the differently ordered evaluation: the rotation through the matrix"""
    q = a[:, :4] * np.array([-1., -1, -1, 1])
    c = -1.0 / a[:, 7:8]
    return np.concatenate([q, rotate_by_matrix(q, c * a[:, 4:7]), 1.0 / a[:, 7:8]], 1)


def sim3_map_plain(a, p):
    return a[:, 7:8] * K.rotate_ref(a[:, :4], p) + a[:, 4:7]


def sim3_map_by_matrix(a, p):
    return a[:, 7:8] * rotate_by_matrix(a[:, :4], p) + a[:, 4:7]


def sim3_log_inputs(exp):
    """class -> n x 8 from `exp` (a function n x 7 -> n x 8: the restatement's or the device's exponential): the exponentials of
    sim3_log_sources(), and `products`, 60 products of two of large_large's whose angle stays within 3.0 (log's factor
    theta / (2 sqrt(1 - d^2)) has a pole at pi, as g2o's has)"""
    src = sim3_log_sources()
    out = {name: exp(u) for name, u in src.items()}
    big = out["large_large"]
    prod = sim3_mul_plain(big[:-1], big[1:])
    keep = [i for i, S in enumerate(prod) if -1 < log_d(S) and math.acos(log_d(S)) <= 3.0 and not any(log_branches(S))]
    out["products"] = prod[keep[:60]]
    return out


def sim3_log_unit(S):
    """eps max(1, |inputs|), over sqrt(1 - d^2) where omega comes from acos(d): d carries eps and acos' slope there is 1 / sqrt(1 - d^2)"""
    d = log_d(S)
    unit = EPS * max(1.0, float(np.abs(S).max()))
    return unit if d > 1 - THRESH else unit / math.sqrt(1 - d * d)


def sim3_log_worst(inputs, got):
    """`inputs` n x 8, `got` n x 7: the worst error of got against the closed form of the branches the header takes"""
    return max(err_units(g, sim3_log_form(S, *log_branches(S)), sim3_log_unit(S)) for S, g in zip(inputs, got))


# ---- lu3_solve
LU3_PATHS = ((0, False), (0, True), (1, False), (1, True), (2, False), (2, True))       # (row of the first pivot, second step swaps)


def _dyadic(f, max_den=2 ** 20):
    f = Fraction(f)
    return f.denominator & (f.denominator - 1) == 0 and f.denominator <= max_den and abs(f.numerator) < 2 ** 40


def lu3_exact(A, b):
    """Eigen's PartialPivLU on Fractions by the header's rule (strict '>': the first of equals wins).  Returns (path, tie, x, dyadic):
    whether some pivot choice had a tie in |entry| and whether every stored value of the elimination and both substitutions is a
    dyadic number of few bits, so that doubles compute the same exactly"""
    m = [[Fraction(v) for v in row] for row in A]
    perm, tie, ok, path = [0, 1, 2], False, True, []
    for k in range(3):
        big = k
        for i in range(k + 1, 3):
            if abs(m[i][k]) > abs(m[big][k]):
                big = i
        tie = tie or sum(abs(m[i][k]) == abs(m[big][k]) for i in range(k, 3)) > 1
        path.append(big)
        if big != k:
            m[k], m[big] = m[big], m[k]
            perm[k], perm[big] = perm[big], perm[k]
        if m[k][k] == 0:
            return None
        for i in range(k + 1, 3):
            m[i][k] /= m[k][k]
            ok = ok and _dyadic(m[i][k])
        for i in range(k + 1, 3):
            for j in range(k + 1, 3):
                m[i][j] -= m[i][k] * m[k][j]
                ok = ok and _dyadic(m[i][j])
    y = [Fraction(0)] * 3
    for i in range(3):
        y[i] = Fraction(b[perm[i]]) - sum(m[i][j] * y[j] for j in range(i))
        ok = ok and _dyadic(y[i])
    x = [Fraction(0)] * 3
    for i in (2, 1, 0):
        s = y[i]
        for j in range(i + 1, 3):
            s -= m[i][j] * x[j]
            ok = ok and _dyadic(s)
        x[i] = s / m[i][i]
        ok = ok and _dyadic(x[i])
    return (path[0], path[1] != 1), tie, x, ok


@cached
def lu3_systems():
    """dict(A n x 9, b n x 3, x n x 3 exact, path, tie): dyadic systems P^T L U (unit lower L with |entries| <= 1, pivots +-2^k) times
    dyadic x, kept when the elimination by the header's rule stays dyadic, 40 of each of the six pivot paths"""
    rng = np.random.default_rng(2103)
    mult = [Fraction(v, 4) for v in range(-4, 5)]
    per, rows = {p: 0 for p in LU3_PATHS}, []
    while min(per.values()) < 40:
        L = [[Fraction(1), 0, 0], [mult[rng.integers(9)], Fraction(1), 0], [mult[rng.integers(9)], mult[rng.integers(9)], Fraction(1)]]
        U = [[Fraction(0)] * 3 for _ in range(3)]
        for i in range(3):
            U[i][i] = Fraction(2) ** int(rng.integers(-2, 3)) * int(rng.choice([-1, 1]))
            for j in range(i + 1, 3):
                U[i][j] = Fraction(int(rng.integers(-8, 9)), 2)
        LUm = [[sum(L[i][k] * U[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        order = rng.permutation(3)
        A = [LUm[int(o)] for o in order]
        x = [Fraction(int(rng.integers(-16, 17)), 4) for _ in range(3)]
        b = [sum(A[i][j] * x[j] for j in range(3)) for i in range(3)]
        res = lu3_exact(A, b)
        if res is None or not res[3] or per[res[0]] >= 40:
            continue
        assert res[2] == x
        per[res[0]] += 1
        rows.append((A, b, x, res[0], res[1]))
    f = lambda v: np.array([[float(c) for c in np.ravel(np.array(r[v], object))] for r in rows])
    return dict(A=f(0), b=f(1), x=f(2), path=[r[3] for r in rows], tie=np.array([r[4] for r in rows]))


@cached
def lu3_rounded():
    """(A, b): NCLASS random systems, where the order of operations shows in the bits"""
    rng = np.random.default_rng(2104)
    return rng.normal(size=(NCLASS, 9)), rng.normal(size=(NCLASS, 3))


def lu3_plain(A, b, pivot=True):
    """the header's elimination on doubles; pivot=False: the differently ordered evaluation, rows taken as they come"""
    out = np.empty((len(A), 3))
    for n, (mm, bb) in enumerate(zip(A, b)):
        m, perm = [[float(v) for v in mm[3 * i:3 * i + 3]] for i in range(3)], [0, 1, 2]
        for k in range(3):
            big, bv = k, abs(m[k][k])
            for i in range(k + 1, 3):
                if pivot and abs(m[i][k]) > bv:
                    bv, big = abs(m[i][k]), i
            if big != k:
                m[k], m[big] = m[big], m[k]
                perm[k], perm[big] = perm[big], perm[k]
            for i in range(k + 1, 3):
                m[i][k] /= m[k][k]
            for i in range(k + 1, 3):
                for j in range(k + 1, 3):
                    m[i][j] -= m[i][k] * m[k][j]
        y, x = [0.] * 3, [0.] * 3
        for i in range(3):
            s = float(bb[perm[i]])
            for j in range(i):
                s -= m[i][j] * y[j]
            y[i] = s
        for i in (2, 1, 0):
            s = y[i]
            for j in range(i + 1, 3):
                s -= m[i][j] * x[j]
            x[i] = s / m[i][i]
        out[n] = x
    return out


@cached
def lu3_zero_column():
    """systems whose first column is zero: bv == 0 skips the division and the result is not finite; the restatement's is the reference"""
    rng = np.random.default_rng(2105)
    A = rng.integers(-4, 5, (20, 3, 3)).astype(np.float64)
    A[:, :, 0] = 0
    return A.reshape(-1, 9), rng.integers(-4, 5, (20, 3)).astype(np.float64)


# ====================================================================================== C. csrc/svd_jacobi.hpp
SVD_SHAPES = {"3x3": (3, 3, 3, True), "4x4": (4, 4, 4, False), "16x9": (16, 9, 9, False), "9x8": (9, 8, 9, True)}
SVD_CLASSES = ("random", "rank_deficient", "zero", "three_i", "equal_values", "scale_p40", "scale_m40", "scale_m70", "denormal")
SVD_NULL_SHAPES = ("4x4", "16x9")
SVD_N = NCLASS
MIN_GAP = 1e-3


def selection_sort(norms):
    """OpenCV's sort of the singular values, from its description: for i = 0 .. n - 2 the first largest of positions i .. n - 1 (a later
    one replaces it only when strictly larger) changes places with position i.  Returns the order: position -> original column."""
    w, order = [float(v) for v in norms], list(range(len(norms)))
    for i in range(len(w) - 1):
        j = max(range(i, len(w)), key=lambda c: (w[c], -c))
        w[i], w[j], order[i], order[j] = w[j], w[i], order[j], order[i]
    return order


def _orthonormal_columns(rng, M, N):
    Q, _ = np.linalg.qr(rng.normal(size=(M, M)))
    return Q[:, :N]


@cached
def svd_inputs(shape, cls):
    """n x N1 x M float: the transposed inputs (row i is column i of the M x N matrix A), storage rows zero"""
    M, N, N1, _ = SVD_SHAPES[shape]
    rng = np.random.default_rng(2200 + 10 * list(SVD_SHAPES).index(shape) + SVD_CLASSES.index(cls))
    if cls in ("random", "scale_p40", "scale_m40", "scale_m70", "denormal"):
        n = 2 * SVD_N if cls == "random" else 20
        A = rng.uniform(-1, 1, (n, M, N))
        if cls == "random":
            A *= 2.0 ** rng.integers(-3, 4, (n, 1, 1))
            if shape in SVD_NULL_SHAPES:       # the null-vector users: the last gap at least MIN_GAP sigma_1, with room for float rounding
                s = np.linalg.svd(A.astype(np.float32).astype(np.float64), compute_uv=False)
                A = A[(s[:, -2] - s[:, -1]) >= 2 * MIN_GAP * s[:, 0]]
            A = A[:SVD_N]                      # SVD_N of them behind the filter
        else:
            A *= 2.0 ** {"scale_p40": 40, "scale_m40": -40, "scale_m70": -70, "denormal": -130}[cls]
    elif cls == "rank_deficient":
        A = rng.integers(-4, 5, (40, M, N)).astype(np.float64)
        A[:, :, N - 1] = A[:, :, 0]
        A[20:, :, 1] = A[20:, :, 0]
    elif cls == "zero":
        A = np.zeros((1, M, N))
    elif cls == "three_i":
        A = np.zeros((1, M, N))
        A[0, :N, :N] = 3 * np.eye(N)
    else:
        # equal singular values, orthogonal columns out of order: signed unit vectors times (2, 1, 2, 1, ...), then all equal: the
        # selection sort's strict '<' must keep the first of equals in front
        A = np.zeros((2, M, N))
        for c in range(N):
            A[0, (c * 7 + 1) % M if M > N else (N - 1 - c), c] = (2.0 if c % 2 else 1.0) * (-1) ** c
            A[1, N - 1 - c, c] = 2.0 * (-1) ** c
    At = np.zeros((len(A), N1, M), np.float32)
    At[:, :N] = np.swapaxes(A, 1, 2).astype(np.float32)
    return At


def svd_unrotated_expected(shape, cls):
    """(W, Vt) of a class whose columns are orthogonal, so that no pair rotates: the columns' norms in the order of selection_sort and
    the rows of the identity in that order -- stated without the restatement"""
    M, N, N1, _ = SVD_SHAPES[shape]
    At = svd_inputs(shape, cls)
    W, Vt = np.zeros((len(At), N), np.float32), np.zeros((len(At), N, N), np.float32)
    for s, at in enumerate(At.astype(np.float64)):
        norms = np.sqrt((at[:N] * at[:N]).sum(1))
        order = selection_sort(norms)
        W[s] = norms[order]
        Vt[s, np.arange(N), order] = 1
    return W, Vt


def svd_measures(shape, At, W, Vt, out, device):
    """The worst ratios over the matrices, in units of FLT_EPSILON, against numpy.linalg.svd of the float input in double:
    w |W - sigma| / sigma_1, vt |Vt Vt^T - I|, a |U diag(W) Vt - A| / sigma_1, u |U^T U - I| over all N1 rows when WANT_U, null the
    angle of the last row of Vt to numpy's times gap / sigma_1 (the two null-vector users); and `descending`.  Where U was not asked
    for the device leaves U diag(W) in At; the restatement has no such switch and always makes U."""
    M, N, N1, want_u = SVD_SHAPES[shape]
    want_u = want_u or not device
    r = dict(w=0.0, vt=0.0, a=0.0, u=0.0, null=0.0, descending=True)
    for at, w, vt, o in zip(At.astype(np.float64), W.astype(np.float64), Vt.astype(np.float64), out.astype(np.float64)):
        A = at[:N].T
        _, s, vh = np.linalg.svd(A)
        s1 = s[0] if s[0] > 0 else 1.0
        r["w"] = max(r["w"], np.abs(w - s).max() / s1 / FEPS)
        r["vt"] = max(r["vt"], np.abs(vt @ vt.T - np.eye(N)).max() / FEPS)
        UW = o[:N].T * w if want_u else o[:N].T
        r["a"] = max(r["a"], np.abs(UW @ vt - A).max() / s1 / FEPS)
        if want_u:
            r["u"] = max(r["u"], np.abs(o @ o.T - np.eye(N1)).max() / FEPS)
        if shape in SVD_NULL_SHAPES and s[0] > 0 and s[-2] - s[-1] >= MIN_GAP * s[0]:
            c = min(1.0, abs(float(vt[-1] @ vh[-1])))
            angle = math.atan2(math.sqrt(max(0.0, 1 - c * c)), c) if c < 0.9 else float(np.linalg.norm(vt[-1] - np.sign(vt[-1] @ vh[-1]) * vh[-1]))
            r["null"] = max(r["null"], angle * (s[-2] - s[-1]) / s[0] / FEPS)
        r["descending"] = r["descending"] and bool((np.diff(w) <= 0).all())
    return r


SVD_RATIOS = ("w", "vt", "a", "u", "null")
SVD_FLOOR = 16.0


# ====================================================================================== D. csrc/front_solve.hpp
# (R, nown, nb): n = R (nown + nb) below, at and above the 16-row and 16-column strides, above 256 once; (6, 0, 3) has k == 0
FRONT_SHAPES = ((6, 1, 0), (6, 1, 1), (7, 1, 1), (7, 2, 0), (6, 2, 1), (7, 3, 5), (6, 8, 20), (7, 10, 30), (6, 0, 3))
FRONT_ROUNDED_SHAPES = FRONT_SHAPES                       # both classes at every shape
FRONT_PACKED_MAX = 168                                  # (7, 10, 30), n = 280, only in rows of n: its triangle does not fit LDS
FRONT_EXACT_N, FRONT_ROUNDED_N = 6, 8
KAPPA_MAX = 1e8


def front_dims(shape):
    R, nown, nb = shape
    return R * (nown + nb), R * nown


@cached
def front_exact(shape):
    """dict(M nsys x n x n, r nsys x n, L, y): M = L L^T with dyadic L (diagonal 1 or 2, entries multiples of 1/4 up to 3/4, two thirds of
    them zero) and r = L y with small integer y.  M, r, the partial factor, the Schur complement L22 L22^T and L22 y2 are exact
    doubles, and so is every intermediate of the right-looking loop."""
    n, k = front_dims(shape)
    rng = np.random.default_rng(2300 + FRONT_SHAPES.index(shape))
    L = np.tril(rng.integers(-3, 4, (FRONT_EXACT_N, n, n)) / 4.0 * (rng.random((FRONT_EXACT_N, n, n)) < 1 / 3), -1)
    L[:, np.arange(n), np.arange(n)] = rng.choice([1.0, 2.0], (FRONT_EXACT_N, n))
    y = rng.integers(-4, 5, (FRONT_EXACT_N, n)).astype(np.float64)
    M = L @ np.swapaxes(L, 1, 2)
    r = np.einsum("sij,sj->si", L, y)
    return dict(M=M, r=r, L=L, y=y)


def front_exact_expected(shape):
    """(lower triangle behind the call, r behind the call): columns [0, k) hold L, the trailing block L22 L22^T, r = (y1, L22 y2)"""
    n, k = front_dims(shape)
    c = front_exact(shape)
    L, y = c["L"], c["y"]
    F = L.copy()
    F[:, k:, k:] = np.tril(L[:, k:, k:] @ np.swapaxes(L[:, k:, k:], 1, 2))
    r = y.copy()
    r[:, k:] = np.einsum("sij,sj->si", L[:, k:, k:], y[:, k:])
    return F, r


@cached
def front_rounded(shape):
    """dict(M, r, kappa): random symmetric positive definite systems Q diag(1 .. 1/kappa) Q^T with kappa from 1e2 to KAPPA_MAX"""
    n, k = front_dims(shape)
    rng = np.random.default_rng(2350 + FRONT_SHAPES.index(shape))
    Ms, kap = [], []
    for s in range(FRONT_ROUNDED_N):
        kappa = 10.0 ** (2 + 6 * s / (FRONT_ROUNDED_N - 1))
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        M = (Q * np.geomspace(1, 1 / kappa, n)) @ Q.T
        Ms.append((M + M.T) / 2)
        kap.append(float(np.linalg.cond(Ms[-1])))
    return dict(M=np.array(Ms), r=rng.normal(size=(FRONT_ROUNDED_N, n)), kappa=np.array(kap))


def front_sequential(M, k, r):
    """The right-looking loop one entry at a time in increasing kk, as every thread of front_partial_llt updates its entries: (F, r,
    ok) with F's lower triangle factored and the upper one untouched; a failing pivot stops the loop where the kernel stops"""
    F, r = np.array(M, np.float64), np.array(r, np.float64)
    n = len(r)
    for kk in range(k):
        d = F[kk, kk]
        if not d > 0 or not np.isfinite(d):
            return F, r, False
        F[kk, kk] = lkk = np.sqrt(d)
        F[kk + 1:, kk] = F[kk + 1:, kk] / lkk
        r[kk] = r[kk] / lkk
        c = F[kk + 1:, kk]
        upd = F[kk + 1:, kk + 1:] - np.outer(c, c)
        F[kk + 1:, kk + 1:] = np.where(np.tri(n - kk - 1, dtype=bool), upd, F[kk + 1:, kk + 1:])
        r[kk + 1:] = r[kk + 1:] - c * r[kk]
    return F, r, True


def front_left_looking(M, k, r):
    """the differently ordered evaluation: every entry's products summed first and subtracted once (the inner-product form)"""
    F, r = np.array(M, np.float64), np.array(r, np.float64)
    n = len(r)
    for j in range(n):
        m = min(j, k)
        for i in range(j, n):
            F[i, j] = F[i, j] - float(np.sum(F[i, :m] * F[j, :m]))
        if j < k:
            F[j, j] = np.sqrt(F[j, j])
            F[j + 1:, j] = F[j + 1:, j] / F[j, j]
    for i in range(n):
        m = min(i, k)
        r[i] = r[i] - float(np.sum(F[i, :m] * r[:m]))
        if i < k:
            r[i] = r[i] / F[i, i]
    return F, r


def front_mp_plan(shape):
    """(the systems of front_rounded(shape) that get the 50-digit reference, the rows of the Schur complement it covers): everything up
    to n = 56; at n = 168 and 280 the systems of the smallest and the largest kappa, L11, L21 and r whole and every seventh row of the
    Schur complement (7 and the strides of 16 have no common factor) with the last, which keeps a test at a few seconds.  The bit
    equality with the sequential loop covers every entry of every system at every shape."""
    n, k = front_dims(shape)
    if n <= 56:
        return list(range(FRONT_ROUNDED_N)), None
    return [0, FRONT_ROUNDED_N - 1], sorted(set(range(k, n, 7)) | {n - 1})


def front_mp(M, k, r, schur_rows=None):
    """the partial factorisation at 50 digits in its inner-product form: (F, r) as lists of mpf, F's lower triangle; schur_rows: the
    rows of the trailing block to compute (None: all), the others are left None"""
    n = len(r)
    m = [[MP.mpf(float(M[i][j])) for j in range(i + 1)] for i in range(n)]
    F = [[MP.mpf(0) if j > i else None for j in range(n)] for i in range(n)]
    rr = [MP.mpf(float(v)) for v in r]
    for j in range(k):
        Lj = F[j][:j]
        F[j][j] = MP.sqrt(m[j][j] - MP.fdot(Lj, Lj))
        for i in range(j + 1, n):
            F[i][j] = (m[i][j] - MP.fdot(F[i][:j], Lj)) / F[j][j]
    for i in range(k):
        rr[i] = (rr[i] - MP.fdot(F[i][:i], rr[:i])) / F[i][i]
    for i in range(k, n):
        rr[i] = rr[i] - MP.fdot(F[i][:k], rr[:k])
    for i in (range(k, n) if schur_rows is None else schur_rows):
        for j in range(k, i + 1):
            F[i][j] = m[i][j] - MP.fdot(F[i][:k], F[j][:k])
    return F, rr


def front_numpy(M, k, r):
    """numpy.linalg.cholesky and solves: L11, L21 = M21 L11^-T, the Schur complement, L11^-1 r1 and r2 - L21 y"""
    n = len(r)
    F = np.array(M, np.float64)
    rr = np.array(r, np.float64)
    if k:
        L11 = np.linalg.cholesky(M[:k, :k])
        L21 = np.linalg.solve(L11, M[k:, :k].T).T
        F[:k, :k], F[k:, :k] = L11, L21
        F[k:, k:] = M[k:, k:] - L21 @ L21.T
        rr[:k] = np.linalg.solve(L11, r[:k])
        rr[k:] = r[k:] - L21 @ rr[:k]
    return F, rr


def front_parts(F, r, k):
    """the four things the callers use: L11, L21, the Schur complement (lower triangles), r"""
    F = np.asarray(F)
    return dict(L11=np.tril(F[:k, :k]), L21=F[k:, :k], schur=np.tril(F[k:, k:]), r=np.asarray(r))


def front_ratio(got, want_mp, kappa):
    """max |got - want| / (eps kappa max(1, max |want|)) over an array, want at 50 digits (entries it leaves None are not compared)"""
    got = np.asarray(got, np.float64)
    pairs = [(g, w) for g, w in zip(got.ravel(), np.array(want_mp, object).reshape(got.shape).ravel()) if w is not None]
    if not pairs:
        return 0.0
    scale = max(1.0, max(float(abs(w)) for _, w in pairs))
    return max(float(abs(MP.mpf(float(g)) - w)) for g, w in pairs) / (EPS * kappa * scale)


FRONT_FLOOR = 4.0
FRONT_FAIL_SHAPES = ((6, 2, 1), (7, 3, 5))
FRONT_FAIL_KINDS = ("zero", "negative", "nan", "inf")


@cached
def front_failing(shape):
    """list of (name, column, M, r): an exact system whose pivot at `column` (0, the middle, k - 1) is the first that is zero, negative,
    NaN or infinite"""
    n, k = front_dims(shape)
    c = front_exact(shape)
    out = []
    for col in (0, k // 2, k - 1):
        for s, kind in enumerate(FRONT_FAIL_KINDS):
            M = c["M"][s].copy()
            lcc = c["L"][s][col, col]
            M[col, col] = {"zero": M[col, col] - lcc * lcc, "negative": M[col, col] - lcc * lcc - 1, "nan": np.nan, "inf": np.inf}[kind]
            out.append(("%s@%d" % (kind, col), col, M, c["r"][s].copy()))
    return out


BACK_SENTINEL = -12345.678


@cached
def front_back_cases(shape, rounded):
    """dict(vtx, xt, F, r, x_own): systems for front_substitute_back of one shape.  vtx scatters the front's vertices over nown + nb + 3
    vertices; xt holds the boundary's solution (small dyadic numbers) and BACK_SENTINEL everywhere else; F is the factor (exact: the
    dyadic L of front_exact, where x_own is dyadic and r = L11^T x_own + L21^T x_b exactly; rounded: numpy's factor of front_rounded
    and a random r, x_own None)"""
    R, nown, nb = shape
    n, k = front_dims(shape)
    rng = np.random.default_rng(2400 + FRONT_SHAPES.index(shape) + 50 * rounded)
    if rounded:
        c = front_rounded(shape)
        F = np.array([np.tril(front_numpy(M, k, r)[0]) for M, r in zip(c["M"], c["r"])])
        for f, M in zip(F, c["M"]):
            f[k:, k:] = np.tril(M[k:, k:])
    else:
        F = front_exact(shape)["L"].copy()
    nsys, nvert = len(F), nown + nb + 3
    vtx = np.array([rng.permutation(nvert)[:nown + nb] for _ in range(nsys)], np.int32)
    xt = np.full((nsys, nvert, R), BACK_SENTINEL)
    xb = rng.integers(-8, 9, (nsys, nb, R)) / 2.0
    for s in range(nsys):
        xt[s, vtx[s, nown:]] = xb[s]
    if rounded:
        r, x_own = rng.normal(size=(nsys, n)), None
    else:
        x_own = rng.integers(-8, 9, (nsys, k)) / 2.0
        r = np.zeros((nsys, n))
        r[:, :k] = np.einsum("sji,sj->si", F[:, :k, :k], x_own) + np.einsum("sji,sj->si", F[:, k:, :k], xb.reshape(nsys, -1))
        r[:, k:] = rng.normal(size=(nsys, n - k))
    return dict(vtx=vtx, xt=xt, F=F, r=r, x_own=x_own, xb=xb.reshape(nsys, -1))


def back_sequential(F, r, xb, k):
    """front_substitute_back's own rows in its order: w = r - sum over j increasing, then the column-wise back substitution"""
    n = len(F)
    w = np.array(r[:k], np.float64)
    for j in range(k, n):
        w = w - F[j, :k] * xb[j - k]
    for kk in range(k - 1, -1, -1):
        w[kk] = w[kk] / F[kk, kk]
        w[:kk] = w[:kk] - F[kk, :kk] * w[kk]
    return w


def back_row_wise(F, r, xb, k):
    """the differently ordered evaluation: every unknown's products summed first (the row-wise back substitution)"""
    w = np.array(r[:k], np.float64) - F[k:, :k].T @ xb
    x = np.zeros(k)
    for i in range(k - 1, -1, -1):
        x[i] = (w[i] - float(np.sum(F[i + 1:k, i] * x[i + 1:]))) / F[i, i]
    return x


def back_mp(F, r, xb, k):
    n = len(F)
    w = [MP.mpf(float(r[i])) - sum(MP.mpf(float(F[j, i])) * MP.mpf(float(xb[j - k])) for j in range(k, n)) for i in range(k)]
    for kk in range(k - 1, -1, -1):
        w[kk] /= MP.mpf(float(F[kk, kk]))
        for i in range(kk):
            w[i] -= MP.mpf(float(F[kk, i])) * w[kk]
    return w


def back_numpy(F, r, xb, k):
    return np.linalg.solve(F[:k, :k].T, r[:k] - F[k:, :k].T @ xb) if k else np.zeros(0)


# ====================================================================================== E. csrc/ba_edges.hpp
CAM = np.array([520.5, 516.25, 318.75, 255.5])      # fx != fy; exact as floats too (the marker restatement takes the camera as floats)
MONO_N = 60


@cached
def mono_inputs():
    """(T n x 7, X n x 3, obs n x 2): poses with unit quaternions (the last has w near 0), points at depths from 0.5 to 50 and off the
    axis, so that every entry of both Jacobians is non-zero"""
    rng = np.random.default_rng(2500)
    q = random_quats(rng, MONO_N)
    q[-1] = np.array([0.6, -0.64, 0.48, 1e-9]) / np.linalg.norm([0.6, -0.64, 0.48, 1e-9])
    t = rng.uniform(-3, 3, (MONO_N, 3))
    depth = np.geomspace(0.5, 50, MONO_N)
    Xc = np.stack([depth * rng.uniform(0.1, 0.5, MONO_N) * rng.choice([-1, 1], MONO_N), depth * rng.uniform(0.1, 0.4, MONO_N) * rng.choice([-1, 1], MONO_N), depth], 1)
    Xw = np.stack([np.array(_rot_matrix(list(qq))).T @ (xc - tt) for qq, xc, tt in zip(q, Xc, t)])
    obs = np.stack([Xc[:, 0] / Xc[:, 2] * CAM[0] + CAM[2], Xc[:, 1] / Xc[:, 2] * CAM[1] + CAM[3]], 1) + rng.normal(0, 1.5, (MONO_N, 2))
    return np.concatenate([q, t], 1), Xw, obs


def rot_of_plain(q):
    """Eigen's toRotationMatrix on doubles in the header's order (numpy): n x 3 x 3"""
    return np.moveaxis(np.array(_rot_matrix([q[:, 0], q[:, 1], q[:, 2], q[:, 3]])), 2, 0)


def rot_of_textbook(q):
    """1 - 2 (y^2 + z^2), 2 (x y - z w), ...: the same bits as rot_of_plain, since doubling is exact; used to build inputs"""
    return np.stack([K.quat_to_matrix(qq) for qq in q])


def rot_of_one_by_one(q):
    """the differently ordered evaluation: the diagonal as (1 - tyy) - tzz instead of 1 - (tyy + tzz)"""
    R = rot_of_plain(q)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    txx, tyy, tzz = (2 * x) * x, (2 * y) * y, (2 * z) * z
    R[:, 0, 0], R[:, 1, 1], R[:, 2, 2] = (1 - tyy) - tzz, (1 - txx) - tzz, (1 - txx) - tyy
    return R


def mono_plain(T, X, obs, cam, variant=False):
    """lba_mono_linearize on doubles in its own order: err, Jp, Jx.  variant: the differently ordered evaluation (x (y / z^2) in Jp,
    -1 / z outside the sum in Jx)"""
    fx, fy = cam[0], cam[1]
    Xc = K.rotate_ref(T[:, :4], X) + T[:, 4:]
    err, _ = K.project_ref(Xc, obs, cam, np.ones(len(X)))
    x, y, z = Xc.T
    z_2 = z * z
    s = -1. / z
    zero = np.zeros_like(x)
    t0 = np.stack([s * fx, s * zero, s * (-x / z * fx)], 1)
    t1 = np.stack([s * zero, s * fy, s * (-y / z * fy)], 1)
    R = rot_of_plain(T[:, :4])
    if variant:
        # -1 / z taken out of the sum (two of the three products are the sum: the third is a zero, so reversing them changes nothing)
        Jx = np.stack([s[:, None] * (fx * R[:, 0] + (-x / z * fx)[:, None] * R[:, 2]), s[:, None] * (fy * R[:, 1] + (-y / z * fy)[:, None] * R[:, 2])], 1)
        Jp = np.stack([np.stack([x * (y / z_2) * fx, -(1 + x * (x / z_2)) * fx, y * fx / z, -fx / z, zero, x * fx / z_2], 1),
                       np.stack([(1 + y * (y / z_2)) * fy, -x * (y / z_2) * fy, -x * fy / z, zero, -fy / z, y * fy / z_2], 1)], 1)
    else:
        Jx = np.stack([t0[:, 0:1] * R[:, 0] + t0[:, 1:2] * R[:, 1] + t0[:, 2:3] * R[:, 2], t1[:, 0:1] * R[:, 0] + t1[:, 1:2] * R[:, 1] + t1[:, 2:3] * R[:, 2]], 1)
        Jp = np.stack([np.stack([x * y / z_2 * fx, -(1 + (x * x / z_2)) * fx, y / z * fx, -1. / z * fx, zero, x / z_2 * fx], 1),
                       np.stack([(1 + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy, zero, -1. / z * fy, y / z_2 * fy], 1)], 1)
    return err, Jp, Jx


def _mp_small_exp(delta6):
    """exp of the 4 x 4 generator of a step of 1e-20: four Taylor terms are exact to 1e-100"""
    G = MP.zeros(4)
    O = _skew(delta6[:3])
    for i in range(3):
        for j in range(3):
            G[i, j] = O[i][j]
        G[i, 3] = delta6[3 + i]
    G2 = G * G
    return MP.eye(4) + G + G2 / 2 + G2 * G / 6 + G2 * G2 / 24


def _mp_project(p, cam):
    return [p[0] / p[2] * MP.mpf(float(cam[0])) + MP.mpf(float(cam[2])), p[1] / p[2] * MP.mpf(float(cam[1])) + MP.mpf(float(cam[3]))]


def _mp_central(f, nvar, h=MP.mpf(10) ** -20):
    """the derivative of f (a list of nvar mpf -> 2 mpf) at 0 by central differences with h = 1e-20 at 50 digits: 2 x nvar floats"""
    J = np.zeros((2, nvar))
    for d in range(nvar):
        e = [MP.mpf(0)] * nvar
        e[d] = h
        plus = f(e)
        e[d] = -h
        minus = f(e)
        for a in range(2):
            J[a, d] = float((plus[a] - minus[a]) / (2 * h))
    return J


def _mp_point(M, p):
    return [M[i, 0] * p[0] + M[i, 1] * p[1] + M[i, 2] * p[2] + M[i, 3] for i in range(3)]


@cached
def mono_true_jacobians():
    """the derivative of obs - pi(exp(delta) T X) in delta (omega first, then upsilon: g2o's order) and in X, from the definition"""
    T, X, obs = mono_inputs()
    Jp, Jx = [], []
    for Ti, Xi, oi in zip(T, X, obs):
        Tm = matrix_of(Ti)
        Xm = [MP.mpf(float(c)) for c in Xi]
        o = [MP.mpf(float(c)) for c in oi]

        def f_pose(d):
            pr = _mp_project(_mp_point(_mp_small_exp(d) * Tm, Xm), CAM)
            return [o[0] - pr[0], o[1] - pr[1]]

        def f_point(d):
            pr = _mp_project(_mp_point(Tm, [Xm[i] + d[i] for i in range(3)]), CAM)
            return [o[0] - pr[0], o[1] - pr[1]]
        Jp.append(_mp_central(f_pose, 6))
        Jx.append(_mp_central(f_point, 3))
    return np.array(Jp), np.array(Jx)


MARKER_N = 40


@cached
def marker_inputs():
    """(Tcw n x 12 float, Twm n x 12 float, p n x 3, obs n x 2): cameras looking at markers 1 to 8 units away, marker corners at
    +-0.1"""
    rng = np.random.default_rng(2501)
    qc, qm = random_quats(rng, MARKER_N), random_quats(rng, MARKER_N)
    Rc, Rm = rot_of_textbook(qc), rot_of_textbook(qm)
    p = rng.choice([-0.1, 0.1], (MARKER_N, 3)) * [1, 1, 0]
    Xc = np.stack([rng.uniform(-0.4, 0.4, MARKER_N), rng.uniform(-0.3, 0.3, MARKER_N), np.ones(MARKER_N)], 1) * np.geomspace(1, 8, MARKER_N)[:, None]
    tm = rng.uniform(-2, 2, (MARKER_N, 3))
    # camera pose such that Rc (Rm p + tm) + tc = Xc
    tc = Xc - np.einsum("nij,nj->ni", Rc, np.einsum("nij,nj->ni", Rm, p) + tm)
    Tcw = np.concatenate([Rc, tc[:, :, None]], 2).astype(np.float32).reshape(-1, 12)
    Twm = np.concatenate([Rm, tm[:, :, None]], 2).astype(np.float32).reshape(-1, 12)
    obs = np.stack([Xc[:, 0] / Xc[:, 2] * CAM[0] + CAM[2], Xc[:, 1] / Xc[:, 2] * CAM[1] + CAM[3]], 1) + rng.normal(0, 1.5, (MARKER_N, 2))
    return Tcw, Twm, p, obs


@cached
def marker_true_jacobians(se3_c, se3_m):
    """the derivative of obs - pi(exp(dc) Tc exp(dm) Tm p) in dc and in dm from the definition; se3_c, se3_m: the poses as the helper
    holds them (tuples of 7-tuples: the normalised quaternions of the float matrices)"""
    _, _, p, obs = marker_inputs()
    Jc, Jm = [], []
    for Tc, Tm, pi, oi in zip(se3_c, se3_m, p, obs):
        Mc, Mm = matrix_of(Tc), matrix_of(Tm)
        pm = [MP.mpf(float(c)) for c in pi]
        o = [MP.mpf(float(c)) for c in oi]

        def f(d, cam_side):
            M = _mp_small_exp(d) * Mc * Mm if cam_side else Mc * _mp_small_exp(d) * Mm
            pr = _mp_project(_mp_point(M, pm), CAM)
            return [o[0] - pr[0], o[1] - pr[1]]
        Jc.append(_mp_central(lambda d: f(d, True), 6))
        Jm.append(_mp_central(lambda d: f(d, False), 6))
    return np.array(Jc), np.array(Jm)


def numeric_jacobian_tolerance(E):
    """test_essential_cpu's: g2o's differences with 1e-9 round to 16 eps E / 2e-9 for values up to E and truncate to h^2 times a third
    derivative of order E"""
    h = 1e-9
    return 16 * EPS * E / 2e-9 + 10 * E * h * h


@cached
def diag_inputs():
    """(J n x 2 x 6, w, r0, r1): Jacobians of the size of the mono edge's, Huber weights, residuals"""
    rng = np.random.default_rng(2502)
    return rng.normal(size=(NCLASS, 2, 6)) * 300, rng.uniform(0.05, 1, NCLASS), rng.normal(size=NCLASS) * 3, rng.normal(size=NCLASS) * 3


def diag_plain(J, w, r0, r1, variant=False):
    """lba_diag_block on doubles in its order: the 21 entries J0a (w J0c) + J1a (w J1c), then J0a r0 + J1a r1.  variant: (J^T J) w"""
    out = []
    for a in range(6):
        for c in range(a, 6):
            out.append((J[:, 0, a] * J[:, 0, c] + J[:, 1, a] * J[:, 1, c]) * w if variant else J[:, 0, a] * (w * J[:, 0, c]) + J[:, 1, a] * (w * J[:, 1, c]))
    for a in range(6):
        out.append(J[:, 0, a] * r0 + J[:, 1, a] * r1)
    return np.stack(out, 1)


@cached
def wave_rows():
    """rows of 64 doubles of mixed sign and magnitude, where the order of the sum shows"""
    rng = np.random.default_rng(2503)
    return rng.normal(size=(NCLASS, 64)) * 10.0 ** rng.integers(-6, 7, (NCLASS, 64))


def butterfly(rows, op):
    """what every lane holds after v = op(v, v of lane ^ off) for off = 32, 16, ... 1: n x 64"""
    v = np.array(rows, np.float64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lane ^ off])
    return v


def left_to_right_sum(rows):
    out = np.zeros(len(rows))
    for c in range(64):
        out = out + rows[:, c]
    return out


@cached
def wave_rows_with_nan():
    """wave_rows() with one NaN a row, at lanes 0, 1, 31, 32, 63, ...: fmax drops a NaN, so the result is the maximum of the others"""
    rows = wave_rows().copy()
    at = np.array([0, 1, 31, 32, 63, 17])[np.arange(len(rows)) % 6]
    rows[np.arange(len(rows)), at] = np.nan
    return rows


# ====================================================================================== the steps the passes share
DINV_N = 65          # a second wave of the probe's workgroup runs with one lane


def dinv_inputs():
    """(Hll packed 00 01 02 11 12 22, lambda, class) of DINV_N systems: the identity with lambda 0; J^T J of two and of six random
    observations (J 2 x 3 each) with lambda = 1e-4 x the largest diagonal entry; J^T J of a single observation, rank 2, plus such a
    lambda -- the shape at which a wrong cofactor shows, since the inverse's large entries are cofactors over a small determinant"""
    rng = np.random.default_rng(2101)
    H, lam, cls = [np.array([1., 0, 0, 1, 0, 1])], [0.0], ["identity"]
    for name, nobs, count in (("two", 2, 22), ("six", 6, 21), ("single", 1, 21)):
        for _ in range(count):
            J = rng.normal(size=(2 * nobs, 3)) * 10 ** rng.uniform(-1, 2)
            A = J.T @ J
            H.append(A[np.triu_indices(3)])
            lam.append(1e-4 * A.diagonal().max())
            cls.append(name)
    assert len(H) == DINV_N
    return np.array(H), np.array(lam), cls


def dinv_full(H6, lam):
    M = np.zeros((len(H6), 3, 3))
    iu = np.triu_indices(3)
    M[:, iu[0], iu[1]] = H6
    M[:, iu[1], iu[0]] = H6
    return M + lam[:, None, None] * np.eye(3)


def dinv_bound(M):
    """|D M - I| of the cofactor inverse in doubles, entry by entry.  With m = max |M_ij|: a cofactor is p - q, |p|, |q| <= m^2, off by
    3 eps m^2; the determinant, three cofactors times an entry, by 20 eps m^3 at most; so an entry of D = C / det by
    3 eps m^2 / |det| + max |M^-1| (2 + 20 g) eps, g = m^3 / |det|, and a row of D M adds three of them times m:
        3 eps (3 g + k (2 + 20 g)),   k = m max |M^-1|, the condition number in the max norm (g <= 81 k^2)"""
    Mm = MP.matrix(M.tolist())
    m = max(abs(Mm[i, j]) for i in range(3) for j in range(3))
    inv = Mm ** -1
    g = m ** 3 / abs(MP.det(Mm))
    k = m * max(abs(inv[i, j]) for i in range(3) for j in range(3))
    return float(3 * EPS * (3 * g + k * (2 + 20 * g))), float(k)


PAIR_NSYS = 5
PAIR_CASES = tuple((nitems, diag) for nitems in (0, 1, 3) for diag in (False, True))


def pair_inputs(nitems, diag):
    """random W_i, W_j (6 x 3), D (3 x 3), bl per item, and accumulators that start non-zero"""
    rng = np.random.default_rng(2200 + 10 * nitems + int(diag))
    Wi, Wj = rng.normal(size=(PAIR_NSYS, nitems, 6, 3)), rng.normal(size=(PAIR_NSYS, nitems, 6, 3))
    return Wi, Wj, rng.normal(size=(PAIR_NSYS, nitems, 3, 3)), rng.normal(size=(PAIR_NSYS, nitems, 3)), rng.normal(size=(PAIR_NSYS, 6, 6)), rng.normal(size=(PAIR_NSYS, 6))


def merge_case(R, seed=2300):
    """desc, cmap, fronts of four nodes: 0 the parent (1 own vertex, 2 boundary), 1 its left child (1 own, boundary mapped {2, 0}: it
    arrives reversed, so the row / column swap runs), 2 its right child (2 own, boundary mapped {0}: the parent's block (0, 0) receives
    both children), 3 a node of the parent's shape with the right child alone.  Every double of every front is random."""
    shapes = ((1, 2), (1, 2), (2, 1), (1, 2))
    off, desc = 0, []
    for nown, nb in shapes:
        n = R * (nown + nb)
        desc.append([off, nown, nb, -1, -1, 0, 0])
        off += n * n + 2 * n
    desc[0][3:] = [1, 2, 0, 2]
    desc[3][3:] = [-1, 2, 0, 2]
    rng = np.random.default_rng(seed + R)
    return np.array(desc, np.int32), np.array([2, 0, 0], np.int32), rng.normal(size=off) * 10 ** rng.uniform(-3, 3, off)


def merge_dense(R, desc, cmap, fronts, node, order=(0, 1)):
    """the same by dense algebra: the child's boundary block made symmetric, scattered by the map, its lower triangle added; children
    in `order`"""
    out = fronts.copy()
    off, nown, nb = desc[node][:3]
    n = R * (nown + nb)
    F, r = out[off:off + n * n].reshape(n, n), out[off + n * n:off + n * n + n]
    for ch in order:
        c = desc[node][3 + ch]
        if c < 0:
            continue
        coff, cown, cnb = desc[c][:3]
        m, ck = R * (cown + cnb), R * cown
        G = fronts[coff:coff + m * m].reshape(m, m)[ck:, ck:]
        G = np.tril(G) + np.tril(G, -1).T
        idx = np.concatenate([R * v + np.arange(R) for v in cmap[desc[node][5 + ch]:desc[node][5 + ch] + cnb]])
        T = np.zeros((n, n))
        T[np.ix_(idx, idx)] = G
        F += np.tril(T)          # the places the child does not reach get + 0.0, which leaves every finite double as it is
        t = np.zeros(n)
        t[idx] = fronts[coff + m * m + ck:coff + m * m + m]
        r += t
    return out


RUN_SUM_THREADS = 256
RUN_SUM_SIZES = (0, 1, RUN_SUM_THREADS - 1, RUN_SUM_THREADS + 1, 3 * RUN_SUM_THREADS + 5)


def run_sum_inputs(n):
    rng = np.random.default_rng(2400 + n)
    return rng.normal(size=n) * 10 ** rng.uniform(-8, 8, n)


def run_sum_strided(v, threads=RUN_SUM_THREADS):
    """another order: thread t adds v[t], v[t + threads], ..; then the same butterfly and waves"""
    part = np.zeros(threads)
    for i, x in enumerate(v):
        part[i % threads] += x
    total = 0.0
    for i, w in enumerate(butterfly(part.reshape(-1, 64), np.add)[:, 0]):
        total = w if i == 0 else total + w
    return total
