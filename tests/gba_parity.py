"""What the GlobalBundleAdjustment parity tests share (test infrastructure): the distance between two results and the spread between
the restatement's two summation orders, from which the tolerance of the GPU parity tests follows (with the rule of
tests/lba_parity.py): tolerance = 10 x spread per quantity, computed once per process, on the CPU alone.  A case on which the two
orders run a different number of accepted trials is left out of the spread and of the comparison; with the seeds of
tests/gba_cases.py none is (tests/test_gba_cpu.py checks that)."""
import gba_build
import gba_cases
from lba_parity import rot_angle, scaled_distance, within, QUANTITIES   # noqa: F401

MAX_NOT_COMPARED = 0.10
NAMES = list(gba_cases.CASES)
_cache = {}


def problem(name):
    if name not in _cache:
        pb = gba_cases.case(name)
        _cache[name] = (pb, gba_build.global_bundle_adjustment(pb, gba_build.INSERTION), gba_build.global_bundle_adjustment(pb, gba_build.DEVICE))
    return _cache[name]


def distance(a, b, pb):
    return scaled_distance(a, b, gba_cases.extent(pb))


def same_path(r0, r1):
    """the two orders accepted the same number of trials: every iteration accepts at most one, and an iteration that accepts none ends
    the call, so the counts of iterations and of trials say it"""
    return bool(r0["result"]["iterations"] == r1["result"]["iterations"] and r0["result"]["trials"] == r1["result"]["trials"])


_spread = None


def spread():
    """The largest distance between the restatement's two orders over the cases on which they run the same path: dict of dR, dt, dX,
    dRm, dtm, `per_case` and `left_out`."""
    global _spread
    if _spread is None:
        worst = dict.fromkeys(QUANTITIES, 0.0)
        per, out = {}, []
        for name in NAMES:
            pb, r0, r1 = problem(name)
            if not same_path(r0, r1):
                out.append(name)
                continue
            per[name] = distance(r0, r1, pb)
            for k in worst:
                worst[k] = max(worst[k], per[name][k])
        _spread = dict(worst, per_case=per, left_out=out)
    return _spread


def tolerance():
    """10 x the spread, per quantity: rotations (radians) and translations (relative to the extent) of the keyframes, the points,
    rotations and translations of the markers"""
    s = spread()
    return {k: 10 * s[k] for k in QUANTITIES}
