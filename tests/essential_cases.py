"""Synthetic OptimizeEssentialGraph problems (test infrastructure): a camera that goes once round a circle and drifts, a loop closure
that puts its last keyframes back onto the truth, and the essential graph between them.  Everything is a dict as
binding.eg_arrays takes it, plus `truth` (nkf x 3 x 4) and `bound` where the case has them.

The drift.  Keyframe k of n sits at angle 2 pi k / n of a circle of radius RADIUS and looks along the tangent; T_k is its true pose.
Odometry errs at every step by a similarity delta_k = (rotation w_k, translation tau_k, scale g): the drifted similarity is
S'_k = delta_k (T_k T_k-1^-1) S'_k-1, S'_0 = T_0, with w_k = rot_step * (AXIS + jitter * u_k), tau_k = trans_step * extent *
(DIR + jitter * v_k), u_k and v_k uniform in [-1, 1]^3 and g = scale_end^(1 / (n - 1)).  The keyframe's pose is the SE3 form [R', t' / s'].

The closure.  The last `n_corrected` keyframes are in CorrectedSim3 with the truth in their own scale, Sim3(R_k, s'_k t_k, s'_k), and in
NonCorrectedSim3 with Sim3(R', t' / s', 1); LoopConnections join the last keyframe with the first three.  The first keyframe is fixed:
its drift is zero.

The bound on the distance to the truth after the optimisation.  A drift that is the same at every step is spread evenly over the ring
by the optimum, which is the truth again: what remains is what the jitter put in, at most n * jitter * step per quantity if every step
erred the same way, and the second-order term of composing n steps, (n * step)^2.  bound = n * jitter * step + (n * step)^2, for
the rotation (radians) and for the translation relative to the extent (trans_step is given relative to it too); the translation of
a pose is -R c, so a rotation left over moves it by that angle times the distance of the centre, at most RADIUS: the translation's
bound has the rotation's times RADIUS / extent on top."""
import numpy as np

RADIUS = 5.0
AXIS = np.array([0.3, 0.9, 0.2]) / np.linalg.norm([0.3, 0.9, 0.2])
DIR = np.array([0.5, 0.1, -0.7]) / np.linalg.norm([0.5, 0.1, -0.7])


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def quat_of(R):
    """x, y, z, w of a rotation matrix"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
    q = np.zeros(4)
    q[i] = 0.25 * s
    q[3] = (R[k, j] - R[j, k]) / s
    q[j] = (R[j, i] + R[i, j]) / s
    q[k] = (R[k, i] + R[i, k]) / s
    return q


def rot_of_quat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sim8(R, t, s):
    return np.concatenate([quat_of(R), t, [s]])


def true_pose(k, n):
    a = 2 * np.pi * k / n
    c = np.array([RADIUS * np.cos(a), 0.2 * np.sin(3 * a), RADIUS * np.sin(a)])
    R = rodrigues(np.array([0, -a, 0.0])) @ rodrigues(np.array([0.1, 0, 0.05]))
    return R, -R @ c


def extent(pb=None):
    return 2 * RADIUS


def compose(a, b):
    """the similarity a after b, each (R, t, s)"""
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def drifted(n, rot_step, trans_step, scale_end, jitter, seed):
    """truth (R, t) and drifted (R', t', s') of the n keyframes"""
    rng = np.random.default_rng(seed)
    g = scale_end ** (1.0 / max(n - 1, 1))
    truth, drift = [], []
    for k in range(n):
        R, t = true_pose(k, n)
        if k == 0:
            S = (R, t, 1.0)
        else:
            w = rot_step * (AXIS + jitter * rng.uniform(-1, 1, 3))
            tau = trans_step * extent() * (DIR + jitter * rng.uniform(-1, 1, 3))
            Rp, tp = truth[-1]
            step = (R @ Rp.T, t - R @ Rp.T @ tp, 1.0)      # T_k T_k-1^-1
            S = compose((rodrigues(w), tau, g), compose(step, drift[-1]))
        truth.append((R, t))
        drift.append(S)
    return truth, drift


def graph_case(n, fixed, edges, corrected, ring_n=24, rot_step=0.004, trans_step=0.002, scale_end=1.0, jitter=0.25, seed=1, n_points=0,
               fix_scale=1, leaf_vertices=0, noncorrected=None, iterations=20):
    """The first n keyframes of a drifting ring of ring_n; edges: (i, j, kind) in insertion order; corrected: positions put back onto
    the truth (CorrectedSim3), also in NonCorrectedSim3 unless `noncorrected` names other positions."""
    truth, drift = drifted(ring_n, rot_step, trans_step, scale_end, jitter, seed)
    truth, drift = truth[:n], drift[:n]
    Tcw = np.zeros((n, 3, 4), np.float32)
    for k, (R, t, s) in enumerate(drift):
        Tcw[k, :, :3] = R
        Tcw[k, :, 3] = t / s
    T64 = Tcw.astype(np.float64)
    noncorrected = list(corrected) if noncorrected is None else list(noncorrected)
    pb = dict(kf_id=np.arange(n, dtype=np.int32) * 3 + 7, Tcw=Tcw, fixed=fixed,
              corrected_pos=np.array(corrected, np.int32), corrected=np.array([sim8(truth[k][0], drift[k][2] * truth[k][1], drift[k][2]) for k in corrected]).reshape(-1, 8),
              noncorrected_pos=np.array(noncorrected, np.int32),
              noncorrected=np.array([sim8(T64[k, :, :3], T64[k, :, 3], 1.0) for k in noncorrected]).reshape(-1, 8),
              edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
              edge_kind=np.array([e[2] for e in edges], np.int32), iterations=iterations, fix_scale=fix_scale, leaf_vertices=leaf_vertices)
    rng = np.random.default_rng(seed + 100)
    X = np.zeros((n_points, 3), np.float32)
    ref = np.zeros(n_points, np.int32)
    for i in range(n_points):
        r = int(rng.integers(0, n))
        Xc = np.array([0, 0, 2.0]) + rng.uniform(-1, 1, 3)
        X[i] = T64[r, :, :3].T @ (Xc - T64[r, :, 3])
        ref[i] = -1 if i % 17 == 5 else r
    pb["x3Dw"], pb["point_ref"] = X, ref
    pb["truth"] = np.array([np.hstack([R, t[:, None]]) for R, t in truth])
    steps = ring_n
    rot = steps * jitter * rot_step + (steps * rot_step) ** 2
    pb["bound"] = dict(rot=rot, trans=steps * jitter * trans_step + (steps * trans_step) ** 2 + rot * RADIUS / extent())
    return pb


def chain_edges(n, skip=()):
    return [(k, k - 1, 1) for k in range(1, n) if k not in skip]


def ring(n=24, n_corrected=4, reach=3, extra=(), **kw):
    """the ring: LoopConnections of the last keyframe to the first three, then per keyframe its parent and its covisibles"""
    edges = [(n - 1, j, 0) for j in range(3)]
    for k in range(1, n):
        edges.append((k, k - 1, 1))
        for d in range(2, reach + 1):
            if k - d >= 0:
                edges.append((k, k - d, 1))
        edges += [e for e in extra if e[0] == k]
    return graph_case(n, 0, edges, list(range(n - n_corrected, n)), ring_n=n, **kw)


def consistent(n=6):
    """every measurement agrees with the estimates: no CorrectedSim3, edges of both kinds"""
    return graph_case(n, 0, chain_edges(n) + [(n - 1, 0, 0), (n - 2, 1, 1)], [], n_points=20)


# The drift of the cases the GPU runs whole.  With the slow drift of the defaults the optimum's chi2 is nearly 0, Gauss-Newton converges
# quadratically and every run of 20 iterations ends at the rounding floor, where whether the last trial is accepted is rounding.  With a
# residual this large at the optimum it converges linearly, and the run ends on a stop rule of Levenberg-Marquardt with a margin: three
# iterations in a row that gain less than a thousandth, each still gaining parts in 1e6 to 1e9 (tests/essential_parity.py checks it).
STRONG = dict(rot_step=0.1, trans_step=0.03)

CASES = {
    # one free vertex and one edge have a zero of chi2: this drift makes the second Gauss-Newton step overshoot, and the run ends on ten
    # rejected trials, each rejected by a third of chi2
    "two": lambda: graph_case(2, 0, [(1, 0, 1)], [1], rot_step=0.1, trans_step=0.05),
    "chain3": lambda: graph_case(3, 0, [(2, 0, 0)] + chain_edges(3), [2], **STRONG),
    "ring24_leaf2": lambda: ring(leaf_vertices=2, n_points=200, **STRONG),
    "ring24_leaf64": lambda: ring(leaf_vertices=64, n_points=200, **STRONG),
    "double_edge": lambda: graph_case(4, 0, [(3, 0, 0), (1, 0, 1), (2, 1, 1), (2, 1, 1), (3, 2, 1), (3, 1, 1)], [3]),
    "leaf_to_fixed": lambda: graph_case(4, 0, [(3, 0, 0), (1, 0, 1), (2, 0, 1), (3, 2, 1)], [3]),
    "fixed_middle": lambda: graph_case(8, 4, [(7, 0, 0)] + chain_edges(8) + [(k, k - 2, 1) for k in range(2, 8)], [7], leaf_vertices=2, **STRONG),
    "far_edge": lambda: ring(leaf_vertices=2, extra=[(20, 5, 1)], **STRONG),
    "isolated": lambda: graph_case(5, 0, [(4, 0, 0), (1, 0, 1), (2, 1, 1), (4, 2, 1)], [4], **STRONG),
    "ring24_scale": lambda: ring(leaf_vertices=2, scale_end=1.1, fix_scale=0, n_points=200, **STRONG),
    "ring24_scale_leaf64": lambda: ring(leaf_vertices=64, scale_end=1.1, fix_scale=0, n_points=200, **STRONG),
    # the free scale under the slow drift: three good iterations, then ten trials in a row rejected by a quarter of chi2 each
    "ring24_scale_slow": lambda: ring(leaf_vertices=2, scale_end=1.1, fix_scale=0, n_points=200),
    "ring48": lambda: ring(n=48, reach=5, leaf_vertices=4, n_points=200, extra=[(40, 9, 1)], rot_step=0.05, trans_step=0.015),
    "ring48_leaf64": lambda: ring(n=48, reach=5, leaf_vertices=64, n_points=200, extra=[(40, 9, 1)], rot_step=0.05, trans_step=0.015),
    # the slow ring of the truth test (tests/test_essential_cpu.py); no GPU test runs it whole
    "ring24_slow": lambda: ring(leaf_vertices=2, n_points=200),
}
INSPECT_CASES = ("two", "chain3", "ring24_leaf2", "ring24_leaf64", "double_edge", "leaf_to_fixed", "fixed_middle", "far_edge", "isolated")
FULL_CASES = ("two", "chain3", "ring24_leaf2", "ring24_leaf64", "ring24_scale", "ring24_scale_leaf64", "ring24_scale_slow", "fixed_middle", "far_edge",
              "isolated", "ring48", "ring48_leaf64")
# the same problem under two plans; ring48_leaf64 is one front of 329 rows, more than any LDS holds: the global-memory factorisation
PAIRS = (("ring24_leaf2", "ring24_leaf64"), ("ring24_scale", "ring24_scale_leaf64"), ("ring48", "ring48_leaf64"))


def not_solved(leaf_vertices=2):
    """Eight keyframes, the fixed one in the middle, the CorrectedSim3 of the last one made of its drifted rotation turned by pi about y,
    the quaternion 0.05 % too long; its neighbours are not corrected, so its spanning-tree and covisibility edges err by that turn.  g2o never
    normalises: the rotation matrix of that quaternion has a trace below -1, acos of log() gives NaN, and with it the errors and
    Jacobians of that keyframe's edges.  Every pivot test of a front that holds them fails, no trial is solved, and the estimates
    stay where they were: twenty iterations of one unsolved trial each, by the Levenberg rules (NaN < 0 is false)."""
    pb = dict(graph_case(8, 4, [(7, 0, 0)] + chain_edges(8) + [(k, k - 2, 1) for k in range(2, 8)], [7], leaf_vertices=leaf_vertices, n_points=30))
    c = pb["corrected"].copy()
    x, y, z, w = pb["noncorrected"][-1, :4]          # the drifted rotation, then the turn: an edge to a neighbour errs by pi
    c[-1, :4] = 1.0005 * np.array([-z, w, x, -y])   # the quaternion product (x, y, z, w) (0, 1, 0, 0)
    pb["corrected"] = c
    return pb
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]
