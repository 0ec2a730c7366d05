"""What the LocalBundleAdjustment parity tests share (test infrastructure): the distance between two results, the gate rule for
decisions that sit on the chi2 threshold, and the spread between the restatement's two summation orders, from which the tolerance
of the GPU parity tests follows: tolerance = 10 x spread, computed once per process."""
import numpy as np

import lba_build
import lba_cases

TH = 5.991
GATE_REL = 1e-6
MAX_NOT_COMPARED = 0.10
NAMES = list(lba_cases.CASES) + list(lba_cases.STALE_CASES)
_cache = {}


def problem(name):
    if name not in _cache:
        pb = lba_cases.case(name)
        _cache[name] = (pb, lba_build.local_bundle_adjustment(pb, lba_build.INSERTION), lba_build.local_bundle_adjustment(pb, lba_build.DEVICE))
    return _cache[name]


def rot_angle(Ra, Rb):
    """max rotation angle between corresponding 3 x 3 blocks (radians), from the Frobenius distance"""
    if len(Ra) == 0:
        return 0.0
    d = np.linalg.norm((Ra.astype(np.float64) - Rb.astype(np.float64)).reshape(len(Ra), -1), axis=1)
    return float(d.max() / np.sqrt(2.0))


def distance(a, b, pb):
    return scaled_distance(a, b, lba_cases.extent(pb))


def scaled_distance(a, b, ex):
    """max |dR|, |dt| / ex, |dX| / ex over the keyframes, the points and the marker poses of two results; ex is the problem's extent"""
    out = dict(dR=rot_angle(a["Tcw"][:, :, :3], b["Tcw"][:, :, :3]), dt=0.0, dX=0.0, dRm=rot_angle(a["Twm"][:, :, :3], b["Twm"][:, :, :3]), dtm=0.0)
    if len(a["Tcw"]):
        out["dt"] = float(np.abs(a["Tcw"][:, :, 3].astype(np.float64) - b["Tcw"][:, :, 3]).max() / ex)
    if len(a["x3Dw"]):
        out["dX"] = float(np.abs(a["x3Dw"].astype(np.float64) - b["x3Dw"]).max() / ex)
    if len(a["Twm"]):
        out["dtm"] = float(np.abs(a["Twm"][:, :, 3].astype(np.float64) - b["Twm"][:, :, 3]).max() / ex)
    return out


def decisions_equal(a, b):
    ra, rb = a["result"], b["result"]
    return bool(np.array_equal(ra["n_level1"], rb["n_level1"]) and ra["n_erase"] == rb["n_erase"] and np.array_equal(a["erase"], b["erase"]))


def gated(ref, other):
    """The gate rule: the case is set aside (True) only when every differing flag belongs to an edge whose restatement chi2 is within
    1e-6 relative of 5.991 at some check.  The first check's flags of `other` are known by their counts alone (the
    library does not return the level-1 bytes): a count may differ by at most the number of edges of its kind near the threshold
    at the first check."""
    chi = ref["chi2"]
    near = np.abs(chi - TH) <= GATE_REL * TH
    diff = np.nonzero(ref["erase"] != other["erase"])[0]
    if not all(near[:, e].any() for e in diff):
        return False
    # the first check's flags of `other` come as counts (mono, marker): a count may differ by no more than the edges of that kind that
    # sit on the threshold at the first check
    nmono = len(ref["erase"])
    room = np.array([near[0, :nmono].sum(), near[0, nmono:].sum()])
    if (np.abs(np.asarray(ref["result"]["n_level1"], np.int64) - np.asarray(other["result"]["n_level1"], np.int64)) > room).any():
        return False
    if len(diff) == 0 and np.array_equal(ref["result"]["n_level1"], other["result"]["n_level1"]):
        return False      # nothing differs: there is nothing to set aside
    return True


_spread = None


def spread():
    global _spread
    if _spread is None:
        _spread = _measure_spread()
    return _spread


def _measure_spread():
    """The largest distance between the restatement's two orders over the cases whose decisions agree: dict of dR, dt, dX, dRm, dtm,
    and `per_case`."""
    worst = dict(dR=0.0, dt=0.0, dX=0.0, dRm=0.0, dtm=0.0)
    per = {}
    for name in NAMES:
        pb, r0, r1 = problem(name)
        if not decisions_equal(r0, r1):
            continue
        d = distance(r0, r1, pb)
        per[name] = d
        for k in worst:
            worst[k] = max(worst[k], d[k])
    return dict(worst, per_case=per)


QUANTITIES = ("dR", "dt", "dX", "dRm", "dtm")


DRIVER = "special"     # the case whose dead marker drives the marker spread: its tolerance is its own


def tolerance(name=None):
    """10 x the spread, per quantity: rotations (radians) and translations (relative to the extent) of the keyframes, the points,
    rotations and translations of the markers.  The marker quantities of every case but DRIVER take the spread over the cases
    without DRIVER; name=None gives the overall figures."""
    s = spread()
    tol = {k: 10 * s[k] for k in QUANTITIES}
    if name is not None and name != DRIVER:
        for k in ("dRm", "dtm"):
            tol[k] = 10 * max([d[k] for n, d in s["per_case"].items() if n != DRIVER] + [0.0])
    return tol


def within(d, tol):
    return all(d[k] <= tol[k] for k in QUANTITIES)
