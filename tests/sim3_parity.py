"""What the Sim3 parity contract (tests/test_sim3_gpu.py) derives from the restatement's side alone: which hypotheses are compared,
which correspondences sit on a gate, and whether a run's sequential decision is clear.  Used on the CPU too (tests/test_sim3_cpu.py
checks that the scenes keep the contract's conditions), so nothing here looks at a device result."""
import numpy as np

GAP = 0.03           # compared: (l1 - l2) > GAP * |l1|
CAP = 0.15           # the excluded share a scene may have
GATE_REL = 1e-4      # a correspondence is "near its gate" when err is within this, relative, of maxError


def ran(want, min_inliers, n_iterations):
    """Iterations the window ran."""
    r = want["result"]
    if want["N"] < min_inliers or want["N"] < 3:
        return 0
    return max(0, min(n_iterations, int(r["max_iterations"])))


def compared(want, k):
    e = want["eig"][:k].astype(np.float64)
    return (e[:, 0] - e[:, 1]) > GAP * np.abs(e[:, 0])


def errors64(want, sc, k):
    """err1, err2 (k x N) of every hypothesis in float64 from the restatement's s12, R12, t12 and its float X3Dc / P*im*."""
    s = want["s12"][:k].astype(np.float64); R = want["R12"][:k].astype(np.float64); t = want["t12"][:k].astype(np.float64)
    X1 = want["X3Dc1"].astype(np.float64); X2 = want["X3Dc2"].astype(np.float64)
    P1 = want["P1im1"].astype(np.float64); P2 = want["P2im2"].astype(np.float64)
    K1 = np.asarray(sc["K4_1"], np.float64); K2 = np.asarray(sc["K4_2"], np.float64)
    with np.errstate(all="ignore"):
        A = s[:, None, None] * np.einsum("hij,nj->hni", R, X2) + t[:, None, :]                 # points of 2 in camera 1
        B = np.einsum("hji,hnj->hni", R, X1[None] - t[:, None, :]) / s[:, None, None]          # points of 1 in camera 2
        a = A[..., :2] / A[..., 2:3] * K1[:2] + K1[2:]
        b = B[..., :2] / B[..., 2:3] * K2[:2] + K2[2:]
        e1 = ((P1[None] - a) ** 2).sum(-1); e2 = ((b - P2[None]) ** 2).sum(-1)
    return e1, e2


def near_gate(want, sc, k):
    """k x N bools: the correspondence's err1 or err2 lies within GATE_REL (relative) of its maxError."""
    e1, e2 = errors64(want, sc, k)
    m1 = want["maxError1"].astype(np.float64)[None]; m2 = want["maxError2"].astype(np.float64)[None]
    with np.errstate(all="ignore"):
        return (np.abs(e1 - m1) <= GATE_REL * m1) | (np.abs(e2 - m2) <= GATE_REL * m2)


def decision_reason(want, sc, min_inliers, n_iterations, best_in=0):
    """None when the scan's decisions are clear on the restatement's side, else why not.  Clear: every hypothesis up to the winner
    (all of them when nothing is found) is compared and either has no correspondence near a gate, or cannot reach the running best
    whatever those correspondences do."""
    k = ran(want, min_inliers, n_iterations)
    if k == 0:
        return None
    ok = compared(want, k)
    nn = near_gate(want, sc, k).sum(axis=1)
    best = best_in
    for i in range(k):
        c = int(want["counts"][i])
        if not ok[i]:
            return "hypothesis %d is excluded (eigenvalue gap)" % i
        if nn[i] and c + nn[i] >= best:
            return "hypothesis %d has %d correspondences near a gate, count %d against best %d" % (i, nn[i], c, best)
        if c >= best:
            best = c
            if c > min_inliers:
                return None
    return None
