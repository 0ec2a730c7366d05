"""What the CPU and GPU tests of OptimizeSim3 share: the comparison of two runs' decisions under the project's exclusion rule (the
one of tests/test_pose_opt_gpu.py: a case is "not compared" only when every pair whose flag differs has a restatement chi2 within
1e-6 relative of th2 at some check), and the spread between the restatement's two summation orders over all cases, computed once
per process."""
import numpy as np

import sim3_opt_build as B
import sim3_opt_cases as S

DECISIONS = ("n_correspondences", "n_bad", "more_iterations", "n_inliers")
_refs = {}
_spread = None


def reference(name, order=B.INSERTION):
    """The restatement's run of a case, computed once and shared (do not modify)."""
    if (name, order) not in _refs:
        _refs[name, order] = B.optimize_sim3(S.case(name), order)
    return _refs[name, order]


def decisions(res, match12, ref):
    """("same" | "near gate" | "differ", the indices whose match differs) for a run against the insertion-order restatement."""
    diff = np.flatnonzero(np.asarray(match12) != ref["match12"])
    if not len(diff) and all(res[f] == ref["result"][f] for f in DECISIONS):
        return "same", diff
    th2 = S.TH2

    def near(i):
        c = ref["chi2"][:, i, :]
        c = c[np.isfinite(c)]
        return bool(np.any(np.abs(c - th2) <= 1e-6 * th2))
    return ("near gate" if len(diff) and all(near(i) for i in diff) else "differ"), diff


def order_spread():
    """dict(cases: name -> (max |dR|, |ds| / s, |dt| / extent) between the two summation orders, for the cases whose decisions
    agree; excluded: the names not compared; max: the three maxima)."""
    global _spread
    if _spread is None:
        cases, excluded = {}, []
        for name in S.CASES:
            a, b = reference(name, B.INSERTION), reference(name, B.DEVICE)
            verdict, diff = decisions(b["result"], b["match12"], a)
            assert verdict != "differ", (name, diff[:10], a["result"], b["result"])
            if verdict == "near gate":
                excluded.append(name)
                continue
            cases[name] = S.similarity_difference(b["result"], a["result"], S.case(name)["extent"])
        _spread = dict(cases=cases, excluded=excluded, max=tuple(max(v[k] for v in cases.values()) for k in range(3)))
    return _spread
