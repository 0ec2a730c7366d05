"""GPU tests of OptimizeEssentialGraph (csrc/essential_graph.hip) against the CPU restatement tests/essential_ref.cpp: the stages of
one linearisation and one solve (orbfe_essential_graph_inspect), whole runs within 10 x the spread between the restatement's two vertex
orders (tests/essential_parity.py), the same problem under two elimination plans, equal bits between the host call, the device call and
a repeat, the device call behind a kernel on its stream, and the error conditions of include/orbfe.h."""
import numpy as np
import pytest

import essential_build as B
import essential_cases as S
import essential_parity as P
from pose_opt_device import Dev, Out

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DELTA = 1e-9
_gpu = {}


def gpu_result(orbfe, name):
    if name not in _gpu:
        _gpu[name] = orbfe.optimize_essential_graph(P.problem(name)[0])
    return _gpu[name]


def _dense_system(pb, lin, lam):
    """H + lambda I and b over the free vertices in the caller's order from per-edge errors and Jacobians, in numpy"""
    n = len(pb["Tcw"])
    slot = {v: k for k, v in enumerate([v for v in range(n) if v != pb["fixed"]])}
    H = np.zeros((7 * len(slot), 7 * len(slot))); b = np.zeros(7 * len(slot))
    for e, (i, j) in enumerate(zip(pb["edge_i"], pb["edge_j"])):
        J = {int(i): lin["Ji"][e], int(j): lin["Jj"][e]}
        for u in J:
            if u not in slot:
                continue
            b[7 * slot[u]:7 * slot[u] + 7] -= J[u].T @ lin["err"][e]
            for v in J:
                if v in slot:
                    H[7 * slot[u]:7 * slot[u] + 7, 7 * slot[v]:7 * slot[v] + 7] += J[u].T @ J[v]
    return H + lam * np.eye(len(b)), b, slot


@pytest.mark.parametrize("name", S.INSPECT_CASES)
def test_one_linearisation_and_solve_match_the_restatement(orbfe, name):
    """Tolerances, from the number formats.  An error is a chain of a few dozen double operations on values up to the extent E: 64 eps E.
    A Jacobian entry is the difference of two such errors over 2e-9, each good to 8 eps E: 16 eps E / 2e-9.  A diagonal block and b
    sum over a vertex's d edges 7 products of entries |J| <= Jmax, each entry off by tol_J: d * 7 * 2 * Jmax * tol_J (b: * max |err|, plus
    the error's own tolerance).  x is compared twice: with numpy's solve of the library's OWN linearisation, where only the solver's
    rounding remains, cond * eps * 100; and with the restatement's x, where the Jacobians' tolerance comes through the solve: cond *
    (tol_J / Jmax) * 4 relative to max |x|.  cond is numpy's, of the system without the rows fix_scale leaves empty."""
    pb = S.case(name)
    g, r = orbfe.essential_graph_inspect(pb), B.inspect(pb)
    E = S.extent(pb)
    ne, n = len(pb["edge_i"]), len(pb["Tcw"])
    tol_e = 64 * EPS * E
    tol_J = 16 * EPS * E / (2 * DELTA)
    Jmax = max(np.abs(r["Ji"]).max(), np.abs(r["Jj"]).max(), 1.0)
    deg = np.bincount(np.concatenate([pb["edge_i"], pb["edge_j"]]), minlength=n).max()
    tol_H = deg * 7 * 2 * Jmax * tol_J
    tol_b = deg * 7 * (np.abs(r["err"]).max() * tol_J + Jmax * tol_e)
    d = {k: float(np.abs(g[k] - r[k]).max()) for k in ("err", "Ji", "Jj", "Hd", "b", "x")}
    print(name, d, dict(tol_e=tol_e, tol_J=tol_J, tol_H=tol_H, tol_b=tol_b))
    assert g["solved"] and r["solved"]
    assert d["err"] <= tol_e and d["Ji"] <= tol_J and d["Jj"] <= tol_J and d["Hd"] <= tol_H and d["b"] <= tol_b
    assert abs(g["chi2"] - r["chi2"]) <= 2 * ne * 7 * np.abs(r["err"]).max() * tol_e and g["lambda0"] == 1e-16
    assert not g["Hd"][pb["fixed"]].any() and not g["b"][pb["fixed"]].any() and not g["x"][pb["fixed"]].any()
    for e in range(ne):
        assert not (g["Ji"][e].any() if pb["edge_i"][e] == pb["fixed"] else g["Jj"][e].any() if pb["edge_j"][e] == pb["fixed"] else False)
    H, b, slot = _dense_system(pb, g, g["lambda0"])
    keep = np.ones(len(b), bool)
    if pb["fix_scale"]:
        keep[6::7] = False
    for v, k in slot.items():       # a vertex without an edge holds lambda alone
        if not g["Hd"][v].any():
            keep[7 * k:7 * k + 7] = False
    x_np = np.zeros(len(b))
    x_np[keep] = np.linalg.solve(H[np.ix_(keep, keep)], b[keep])
    cond = np.linalg.cond(H[np.ix_(keep, keep)])
    xg = np.concatenate([g["x"][v] for v in slot]); xr = np.concatenate([r["x"][v] for v in slot])
    xmax = max(np.abs(xr).max(), 1e-300)
    print(name, "cond", cond, "x vs numpy", np.abs(xg - x_np).max(), "x vs restatement", np.abs(xg - xr).max(), "max|x|", xmax)
    assert np.abs(xg - x_np).max() <= 100 * cond * EPS * xmax
    assert np.abs(xg - xr).max() <= 4 * cond * (tol_J / Jmax) * xmax
    assert not xg[~keep].any()


def test_plans_of_the_inspect_cases(orbfe):
    """leaf_vertices = 2 gives the ring of 24 at least three levels and = 64 one front; every free vertex has a node and a place"""
    for name in S.INSPECT_CASES:
        pb = S.case(name)
        g = orbfe.essential_graph_inspect(pb)
        n = len(pb["Tcw"])
        free = [v for v in range(n) if v != pb["fixed"]]
        assert sorted(g["order_of"][free].tolist()) == list(range(n - 1)) and g["order_of"][pb["fixed"]] == -1 and g["node_of"][pb["fixed"]] == -1
        assert int(g["nown"].sum()) == n - 1
    assert orbfe.essential_graph_inspect(S.case("ring24_leaf2"))["nlevels"] >= 3
    one = orbfe.essential_graph_inspect(S.case("ring24_leaf64"))
    assert one["nlevels"] == 1 and one["nown"].tolist() == [23] and one["nb"].tolist() == [0]


def test_whole_runs_match_the_restatement(orbfe):
    """every case at the reference's 20 iterations: outputs within the tolerance, iteration and trial counts equal to the restatement's"""
    print("spread", {k: v for k, v in P.spread().items() if k != "per_case"})
    bad = []
    for name in P.NAMES:
        pb, r0, _ = P.problem(name)
        assert pb["iterations"] == 20
        g = gpu_result(orbfe, name)
        d, tol = P.distance(g, r0, pb), P.tolerance(name)
        res = g["result"]
        print(name, "gpu", (res["iterations"], res["trials"]), "restatement", P.counts(r0), "margin", P.margin(name), d, "tol", tol)
        assert res["status"] == 0
        if not P.within(d, tol):
            bad.append((name, d, tol))
        if (int(res["iterations"]), int(res["trials"])) != P.counts(r0):
            bad.append((name, "counts", (res["iterations"], res["trials"]), P.counts(r0)))
        assert abs(res["chi2_first"] - r0["result"]["chi2_first"]) <= 1e-9 * r0["result"]["chi2_first"]
    assert not bad, bad


@pytest.mark.parametrize("a,b", S.PAIRS)
def test_two_plans_of_one_problem_agree(orbfe, a, b):
    """leaf_vertices 2 (a tree of fronts) and 64 (one front) solve the same systems in two elimination orders"""
    ga, gb = gpu_result(orbfe, a), gpu_result(orbfe, b)
    d = P.distance(ga, gb, S.case(a))
    print(a, b, d, P.tolerance(a))
    assert P.within(d, P.tolerance(a))
    assert (ga["result"]["iterations"], ga["result"]["trials"]) == (gb["result"]["iterations"], gb["result"]["trials"])


def _device_launch(orbfe, pb, inputs=None):
    """enqueue the device call on the null stream; inputs: device addresses that replace uploads of the problem's own arrays.  Returns
    the outputs (guarded device buffers) and what has to stay alive until they are fetched."""
    a = orbfe.eg_arrays(pb)
    nkf, ne, n = len(a["Tcw"]), len(a["edge_i"]), len(a["x3Dw"])
    nbytes = orbfe.essential_graph_scratch_bytes(nkf, ne, n, a["leaf_vertices"])
    assert nbytes > 0
    outs = dict(Tcw_out=Out(np.zeros((nkf, 12), np.float32)), x3Dw_out=Out(np.zeros((max(n, 1), 3), np.float32)), Siw_out=Out(np.zeros((nkf, 8))),
                res=Out(np.zeros(1, orbfe.EG_RESULT_DTYPE)), scratch=Out(np.zeros(nbytes, np.uint8)))
    ptr = {k: v.ptr for k, v in outs.items()}
    ptr["scratch_bytes"] = nbytes
    names = ("Tcw", "corrected_pos", "corrected", "noncorrected_pos", "noncorrected", "x3Dw", "point_ref")
    keep = {k: Dev(a[k]) for k in names if a[k].size and k not in (inputs or {})}
    ptr.update({k: v.ptr for k, v in keep.items()})
    ptr.update(inputs or {})
    orbfe.optimize_essential_graph_device(pb, ptr)
    return outs, keep


def _collect(outs, n):
    outs["scratch"].get()
    return dict(Tcw=outs["Tcw_out"].get().reshape(-1, 3, 4), x3Dw=outs["x3Dw_out"].get()[:n], Siw=outs["Siw_out"].get(), result=outs["res"].get()[0])


def _device_run(orbfe, pb):
    outs, _keep = _device_launch(orbfe, pb)
    return _collect(outs, len(pb["x3Dw"]))


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("Tcw", "x3Dw", "Siw")) and a["result"].tobytes() == b["result"].tobytes()


@pytest.mark.parametrize("name", ["ring24_leaf2", "ring24_scale_leaf64", "ring48"])
def test_device_call_host_call_and_a_repeat_give_equal_bits(orbfe, name):
    """the host call stops enqueueing when the control block says so, the device call enqueues the worst case: the same bits; guard
    bytes around every output and the scratch untouched"""
    pb = P.problem(name)[0]
    host = gpu_result(orbfe, name)
    dev = _device_run(orbfe, pb)
    assert _same_bits(host, dev), (host["result"], dev["result"])
    assert _same_bits(host, orbfe.optimize_essential_graph(pb))
    assert _same_bits(dev, _device_run(orbfe, pb))


def test_device_call_reads_what_a_kernel_on_its_stream_wrote(orbfe):
    """two calls back to back on one stream, nothing fetched in between: the second reads its poses, its points and its CorrectedSim3
    where the first one's last kernel wrote them"""
    pb = P.problem("ring24_leaf2")[0]
    first, keep1 = _device_launch(orbfe, pb)
    rows = pb["corrected_pos"]
    assert rows.tolist() == list(range(rows[0], rows[0] + len(rows)))
    second, keep2 = _device_launch(orbfe, pb, inputs=dict(Tcw=first["Tcw_out"].ptr, x3Dw=first["x3Dw_out"].ptr, corrected=first["Siw_out"].ptr + 64 * int(rows[0])))
    one, two = _collect(first, len(pb["x3Dw"])), _collect(second, len(pb["x3Dw"]))
    assert _same_bits(one, gpu_result(orbfe, "ring24_leaf2"))
    chained = dict(pb, Tcw=one["Tcw"], x3Dw=one["x3Dw"], corrected=one["Siw"][rows])
    assert _same_bits(two, orbfe.optimize_essential_graph(chained))
    assert two["result"]["chi2_first"] != one["result"]["chi2_first"]


def test_a_call_without_edges_or_with_one_keyframe_returns_its_inputs(orbfe):
    pb = dict(S.case("ring24_leaf2"))
    for k in ("edge_i", "edge_j", "edge_kind"):
        pb[k] = np.zeros(0, np.int32)
    out = orbfe.optimize_essential_graph(pb)
    assert np.array_equal(out["Tcw"], pb["Tcw"]) and np.array_equal(out["x3Dw"], pb["x3Dw"]) and out["result"]["iterations"] == 0
    assert np.array_equal(out["Siw"][pb["corrected_pos"]], pb["corrected"])
    one = dict(Tcw=pb["Tcw"][:1], fixed=0, edge_i=[], edge_j=[], edge_kind=[], x3Dw=pb["x3Dw"][:5], point_ref=np.zeros(5, np.int32))
    out = orbfe.optimize_essential_graph(one)
    assert np.array_equal(out["Tcw"], one["Tcw"]) and np.array_equal(out["x3Dw"], one["x3Dw"])


def _refused(orbfe, pb, code):
    """the host call raises with `code` and the library's outputs stay as they were"""
    import ctypes as C
    L = orbfe.load()
    a = orbfe.eg_arrays(pb)
    nkf, n = len(a["Tcw"]), len(a["x3Dw"])
    Tout = np.full((max(nkf, 1), 12), 7.5, np.float32); Xout = np.full((max(n, 1), 3), 7.5, np.float32); Siw = np.full((max(nkf, 1), 8), 7.5)
    res = np.full(1, 0x55, np.uint8).repeat(orbfe.EG_RESULT_DTYPE.itemsize)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = L.orbfe_optimize_essential_graph(*(orbfe._eg_graph_args(a) + [orbfe._ptr_or_none(a["x3Dw"]), orbfe._ptr_or_none(a["point_ref"]), n, a["iterations"],
                                                                       a["fix_scale"], a["leaf_vertices"], p(Tout), p(Xout), p(Siw), p(res), 0]))
    assert rc == code, (rc, L.orbfe_last_error())
    assert (Tout == 7.5).all() and (Xout == 7.5).all() and (Siw == 7.5).all() and (res == 0x55).all()
    return L.orbfe_last_error().decode()


def test_every_refusal_writes_nothing(orbfe):
    base = S.case("ring24_leaf2")

    def with_(**kw):
        pb = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        for k, v in kw.items():
            pb[k] = v(pb[k]) if callable(v) else v
        return pb

    def setat(idx, val):
        def f(a):
            a = a.copy()
            a[idx] = val
            return a
        return f

    INV, CAP = orbfe.ORBFE_ERR_INVALID, orbfe.ORBFE_ERR_CAPACITY
    assert "itself" in _refused(orbfe, with_(edge_j=setat(5, int(base["edge_i"][5]))), INV)
    _refused(orbfe, with_(edge_i=setat(0, 24)), INV)
    _refused(orbfe, with_(edge_j=setat(0, -1)), INV)
    _refused(orbfe, with_(edge_kind=setat(3, 2)), INV)
    _refused(orbfe, with_(corrected_pos=setat(0, 99)), INV)
    _refused(orbfe, with_(noncorrected_pos=setat(1, int(base["noncorrected_pos"][0]))), INV)
    _refused(orbfe, with_(point_ref=setat(7, 24)), INV)
    _refused(orbfe, with_(point_ref=setat(7, -2)), INV)
    _refused(orbfe, with_(Tcw=setat((3, 1, 2), np.nan)), INV)
    _refused(orbfe, with_(corrected=setat((0, 4), np.inf)), INV)
    _refused(orbfe, with_(noncorrected=setat((2, 0), np.nan)), INV)
    _refused(orbfe, with_(x3Dw=setat((9, 1), np.inf)), INV)
    assert "fixed" in _refused(orbfe, with_(fixed=24), INV)
    _refused(orbfe, with_(fixed=-1), INV)
    assert "scale" in _refused(orbfe, with_(corrected=setat((1, 7), 0.0)), INV)
    _refused(orbfe, with_(noncorrected=setat((1, 7), -1.0)), INV)
    _refused(orbfe, with_(iterations=21), INV)
    big = orbfe.EG_MAX_KEYFRAMES + 1
    assert "ORBFE_EG_MAX_KEYFRAMES" in _refused(orbfe, dict(Tcw=np.tile(base["Tcw"][:1], (big, 1, 1)), fixed=0, edge_i=[1], edge_j=[0], edge_kind=[1]), CAP)
    many = orbfe.EG_MAX_EDGES + 1
    assert "ORBFE_EG_MAX_EDGES" in _refused(orbfe, with_(edge_i=np.full(many, 1, np.int32), edge_j=np.zeros(many, np.int32), edge_kind=np.ones(many, np.int32)), CAP)
    assert orbfe.essential_graph_scratch_bytes(big, 10, 0) == 0 and orbfe.essential_graph_scratch_bytes(10, many, 0) == 0
    assert 0 < orbfe.essential_graph_scratch_bytes(orbfe.EG_MAX_KEYFRAMES, orbfe.EG_MAX_EDGES, 100000) < 1e9


def test_a_call_that_is_never_solved_returns_its_estimates(orbfe):
    """tests/essential_cases.not_solved, under a tree of fronts and as one front: a pivot that is not positive in a front, the trial
    judged as not solved, the update kept, the back substitution skipped, parents fed by children that gave up -- twenty iterations of
    one unsolved trial, as the restatement, and the estimates out as they went in"""
    for leaf in (2, 64):
        pb = S.not_solved(leaf)
        g = orbfe.essential_graph_inspect(pb)
        assert not g["solved"] and np.isnan(g["chi2"]) and not g["x"].any()
        out, ref = orbfe.optimize_essential_graph(pb), B.optimize(pb)
        assert (int(out["result"]["iterations"]), int(out["result"]["trials"])) == P.counts(ref) == (20, 20)
        assert np.isnan(out["result"]["chi2_first"]) and out["result"]["status"] == 0
        same = orbfe.optimize_essential_graph(dict(pb, iterations=0))
        for k in ("Siw", "Tcw", "x3Dw"):
            assert np.array_equal(out[k], same[k]), k
        assert P.within(P.distance(out, ref, pb), P.tolerance("fixed_middle"))
        assert _same_bits(out, _device_run(orbfe, pb))


def test_null_pointers_and_alignment_are_refused_by_the_entry_points(orbfe):
    """the library's own checks, not the plan's: the host call without an output or an input it needs, the device call without its
    record, its scratch, or with a scratch off its 256-byte alignment -- each ORBFE_ERR_INVALID before anything is enqueued"""
    import ctypes as C
    L = orbfe.load()
    pb = S.case("chain3")
    a = orbfe.eg_arrays(pb)
    nkf = len(a["Tcw"])
    Tout = np.full((nkf, 12), 7.5, np.float32); Xout = np.full((4, 3), 7.5, np.float32); res = np.zeros(1, orbfe.EG_RESULT_DTYPE)
    X = np.zeros((4, 3), np.float32); ref = np.zeros(4, np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)

    def host(graph=None, x=X, r=ref, tout=Tout, xout=Xout, rs=res):
        args = graph or orbfe._eg_graph_args(a)
        return L.orbfe_optimize_essential_graph(*(args + [p(x), p(r), 4, 20, 1, 0, p(tout), p(xout), None, p(rs), 0]))

    assert host() == 0 and not (Tout == 7.5).all()
    Tout[:] = 7.5
    g = orbfe._eg_graph_args(a)
    for bad in (dict(rs=None), dict(tout=None), dict(xout=None), dict(x=None), dict(r=None), dict(graph=g[:1] + [None] + g[2:]),
                dict(graph=g[:10] + [None] + g[11:]), dict(graph=g[:12] + [None] + g[13:]), dict(graph=g[:5] + [None] + g[6:])):
        assert host(**bad) == orbfe.ORBFE_ERR_INVALID, bad
        assert (Tout == 7.5).all()
    d = Dev(np.zeros(1 << 16, np.uint8))
    nbytes = orbfe.essential_graph_scratch_bytes(nkf, len(a["edge_i"]), 0, 0)
    scratch = Dev(np.zeros(nbytes + 512, np.uint8))
    ok = dict(Tcw=d.ptr, corrected_pos=d.ptr, corrected=d.ptr, noncorrected_pos=d.ptr, noncorrected=d.ptr, Tcw_out=d.ptr + 4096, res=d.ptr + 8192,
              scratch=scratch.ptr, scratch_bytes=nbytes)
    for bad in (dict(res=0), dict(scratch=0), dict(scratch=scratch.ptr + 64), dict(Tcw=0), dict(Tcw_out=0), dict(corrected=0), dict(noncorrected_pos=0)):
        with pytest.raises(orbfe.OrbfeError, match="invalid argument"):
            orbfe.optimize_essential_graph_device(pb, dict(ok, **bad))
    assert not d.get().any()


def test_device_call_reports_what_only_the_device_can_check(orbfe):
    """values on the device: the status comes back in the record and no output is written; a short scratch is refused on the host"""
    pb = dict(S.case("ring24_leaf2"))
    bad = pb["corrected"].copy()
    bad[2, 7] = 0.0
    pb["corrected"] = bad
    out = _device_run(orbfe, pb)
    assert out["result"]["status"] == orbfe.ORBFE_ERR_INVALID and not out["Tcw"].any() and not out["x3Dw"].any() and not out["Siw"].any()
    a = orbfe.eg_arrays(S.case("chain3"))
    d = Dev(np.zeros(4096, np.uint8))
    with pytest.raises(orbfe.OrbfeError, match="scratch"):
        orbfe.optimize_essential_graph_device(S.case("chain3"), dict(Tcw=d.ptr, corrected_pos=d.ptr, corrected=d.ptr, noncorrected_pos=d.ptr,
                                                                     noncorrected=d.ptr, Tcw_out=d.ptr, res=d.ptr, scratch=d.ptr, scratch_bytes=1024))
    assert len(a["Tcw"]) == 3
