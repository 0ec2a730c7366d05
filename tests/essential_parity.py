"""What the OptimizeEssentialGraph parity tests share (test infrastructure): the distance between two results, the spread between the
restatement's two vertex orders, from which the tolerance of the GPU parity tests follows (tolerance = 10 x spread,
computed once per process, nothing typed in by hand), and the condition under which two runs' counts are comparable.

Counts.  The restatement reports the margin of a run: the smallest relative change of chi2 any solved trial was judged on.  A run
whose margin is at the rounding floor (parts in 1e12) ends on rounding: whether its last trial is accepted, has rho == 0 or is the
first of ten rejections is not a property two correct implementations share, nor the restatement's two orders.  So the cases are
built (tests/essential_cases.py) so that every run of the reference's 20 iterations is DECIDED: the margin of both orders is at least
MARGIN = 1e-9, three decades above that floor.  tests/test_essential_cpu.py holds the cases to that and to equal counts in the two
orders; the GPU tests then assert equal counts on every case."""
import numpy as np

import essential_build
import essential_cases

MARGIN = 1e-9
NAMES = essential_cases.FULL_CASES
_cache = {}


def reversed_order(pb):
    n = len(pb["Tcw"])
    return [v for v in range(n) if v != pb["fixed"]][::-1]


def problem(name):
    """the case, and the restatement's results in the caller's order and in the reversed one"""
    if name not in _cache:
        pb = essential_cases.case(name)
        _cache[name] = (pb, essential_build.optimize(pb), essential_build.optimize(pb, reversed_order(pb)))
    return _cache[name]


def margin(name):
    _, r0, r1 = problem(name)
    return min(r0["result"]["margin"], r1["result"]["margin"])


def decided(name):
    return margin(name) >= MARGIN


def counts(r):
    r = r["result"]
    return int(r["iterations"]), int(r["trials"])


def _rot(q):
    q = q / np.linalg.norm(q, axis=1)[:, None]
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)


def _angle(Ra, Rb):
    """max rotation angle between corresponding rotations (radians), from the Frobenius distance"""
    return float(np.linalg.norm(Ra - Rb, axis=1).max() / np.sqrt(2.0)) if len(Ra) else 0.0


QUANTITIES = ("dR", "dt", "ds", "dX", "dRf", "dtf")


def distance(a, b, pb=None):
    """Siw: rotation angle (dR), translation relative to the extent (dt), log-scale (ds).  The float outputs: points (dX) and Tcw's
    translation (dtf) relative to the extent, Tcw's rotation as an angle (dRf)."""
    ex = essential_cases.extent(pb)
    Sa, Sb = np.asarray(a["Siw"], np.float64), np.asarray(b["Siw"], np.float64)
    Ta, Tb = np.asarray(a["Tcw"], np.float64), np.asarray(b["Tcw"], np.float64)
    return dict(dR=_angle(_rot(Sa[:, :4]), _rot(Sb[:, :4])), dt=float(np.abs(Sa[:, 4:7] - Sb[:, 4:7]).max() / ex),
                ds=float(np.abs(np.log(Sa[:, 7]) - np.log(Sb[:, 7])).max()),
                dX=float(np.abs(np.asarray(a["x3Dw"], np.float64) - b["x3Dw"]).max() / ex) if len(a["x3Dw"]) else 0.0,
                dRf=_angle(Ta[:, :, :3].reshape(-1, 9), Tb[:, :, :3].reshape(-1, 9)), dtf=float(np.abs(Ta[:, :, 3] - Tb[:, :, 3]).max() / ex))


def group(name):
    """the regime a case's tolerance comes from: the reference's call (fix_scale) or the free scale with its 1.1 drift"""
    return "fix_scale" if essential_cases.case(name).get("fix_scale", 1) else "free_scale"


_spread = None


def spread():
    """per group the largest distance between the restatement's two orders over its cases: dict group -> dict of QUANTITIES; `per_case`
    beside them"""
    global _spread
    if _spread is None:
        out = {"fix_scale": dict.fromkeys(QUANTITIES, 0.0), "free_scale": dict.fromkeys(QUANTITIES, 0.0), "per_case": {}}
        for name in NAMES:
            pb, r0, r1 = problem(name)
            d = distance(r0, r1, pb)
            out["per_case"][name] = d
            for k in QUANTITIES:
                out[group(name)][k] = max(out[group(name)][k], d[k])
        _spread = out
    return _spread


def float_ulp(name):
    """one unit in the last place of the float outputs, in the units of dX / dtf (relative to the extent) and of dRf (an entry of a
    rotation matrix is below 1)"""
    ex = essential_cases.extent()
    pb = essential_cases.case(name)
    big = max(float(np.abs(pb["Tcw"][:, :, 3]).max()), float(np.abs(pb["x3Dw"]).max()) if len(pb["x3Dw"]) else 0.0, 1.0)
    u = float(np.spacing(np.float32(2 * big))) / ex
    return dict(dX=u, dtf=u, dRf=float(np.spacing(np.float32(1.0))))


def tolerance(name):
    """10 x the spread of the case's group per quantity; a float output whose spread is exactly zero gets one unit in the last place,
    since the final rounding can fall either way"""
    s = spread()[group(name)]
    tol = {k: 10 * s[k] for k in QUANTITIES}
    for k, u in float_ulp(name).items():
        if s[k] == 0.0:
            tol[k] = u
    return tol


def within(d, tol):
    return all(d[k] <= tol[k] for k in QUANTITIES)
