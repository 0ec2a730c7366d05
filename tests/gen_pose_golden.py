"""Writes tests/golden/pose_hard_cases.npz: the hard marker-pose cases of tests/pose_hard_cases.py, their 50-digit reference
(tests/pose_ref.py) stage by stage and as a whole, the envelope of the CPU oracle against that reference and the per-case tolerances
that tests/test_pose_stages_gpu.py and tests/test_pose_gpu.py apply.  Run as  python tests/gen_pose_golden.py ; build() returns the
arrays, and tests/test_pose_ref_cpu.py compares them with the committed file.

Tolerances (written into the file, so that the GPU tests only read them):
  tolR = 4 * (A * eps / (pi - w)^2 + B) + F   per solution: A, B the oracle's envelope measured here (A: the largest
         eR * (pi - w)^2 / eps where pi - w < 1e-2, B: the largest eR elsewhere, both also over the rot2vec stage set evaluated in plain
         doubles, which is the oracle's rot2vec), F the change of the reference rotation when its own rotation vector is rounded to float.
  tolE = 1e-3 * (1 + err) + G * 4 * (A * eps / (pi - w)^2 + B)   for the reprojection stage: the project's 1e-3 px, and the rotation
         tolerance carried to pixels by G = 2 sqrt(2) max(fx, fy) size / t_z (a corner at half a diagonal from the centre, doubled for
         the factor 1 + |x| + |y| of the perspective division).
  W_H, W_rot, W_t, W_ev: the worst error of the plain double evaluation (numpy / LAPACK) in units of eps times the stage's condition;
         the device may reach 4 x that, at least 4 (as tests/test_device_units_gpu.py bounds ldlt_solve)."""
import os

import numpy as np

import oracle_lib
import pose_cases as pc
import pose_hard_cases as hc
import pose_ref as pr
from pose_ref import MP, F64, EPS, FLT_EPS, tofloat

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_hard_cases.npz")
ZONE = 64 * EPS
ENVELOPE_N = 300
ROT2VEC_W = (0.0, 1e-8, 1e-7, 1.2e-7, 1.3e-7, 1e-6, 1e-3, 1.0, np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-8)
ROT2VEC_AXES = ((1.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.3, -0.5, 0.8))


def eR(rvec, R):
    return float(np.abs(pc.rodrigues(rvec) - np.asarray(R, np.float64).reshape(3, 3)).max())


def oracle_against(want, R, t):
    """the oracle's two solutions against the reference's, paired by translation (which rot2vec does not touch): eR per reference
    solution, and the relative difference of the translations"""
    dt = [[np.abs(want[2 * a + 1] - t[b]).max() for b in range(2)] for a in range(2)]
    swap = max(dt[0][1], dt[1][0]) < max(dt[0][0], dt[1][1])
    e = [eR(want[2], R[0]), eR(want[0], R[1])] if swap else [eR(want[0], R[0]), eR(want[2], R[1])]
    return e, min(max(dt[0][1], dt[1][0]), max(dt[0][0], dt[1][1])) / np.abs(t).max()


def rot_condition(rad):
    """rotations(): b = sqrt(radicand) moves by (a few eps) / (2 b)"""
    b = np.sqrt(max(min(rad), ZONE))
    return max(1.0, 1.0 / (2 * b))


def rot2vec_stage_set():
    import mpmath as mp
    R, pimw, zero, edge = [], [], [], []
    for ax in ROT2VEC_AXES:
        a = np.array(ax) / np.linalg.norm(ax)
        for w in ROT2VEC_W:
            R.append(tofloat(pr.rodrigues(MP, [mp.mpf(float(v)) * mp.mpf(w) for v in a])))
    R.append(np.diag([1.0, -1.0, -1.0]).ravel())
    for m in R:
        w = mp.acos((mp.mpf(m[0]) + mp.mpf(m[4]) + mp.mpf(m[8]) - 1) / 2)
        pimw.append(float(mp.pi - w)); zero.append(bool(w < FLT_EPS))
        # 1.2e-7: the argument of acos rounds to 1 - 2^-47 in double, whose arc cosine is FLT_EPSILON (1 + 6e-16): three ulps decide the
        # branch, so either is right there
        edge.append(bool(abs(float(np.arccos((m[0] + m[4] + m[8] - 1.0) / 2.0)) / FLT_EPS - 1) < 64 * EPS))
    return np.array(R), np.array(pimw), np.array(zero), np.array(edge)


def psd_set():
    rng = np.random.default_rng(170)
    out = []
    for i in range(40):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        lam = np.sort(rng.uniform(0.1, 10, 3))
        if i % 4 == 0:
            lam[0] = 0.0                                   # semi-definite
        if i % 4 == 1:
            lam[0] = lam[1] * (1 - 10.0 ** -rng.integers(2, 7))   # a close pair
        s = (Q * lam) @ Q.T
        s = (s + s.T) / 2
        out.append([s[0, 0], s[0, 1], s[0, 2], s[1, 1], s[1, 2], s[2, 2]])
    return np.array(out)


def eig_ratio(h, ref, gap):
    d = min(np.abs(h - ref).max(), np.abs(h + ref).max())
    return d / (EPS / max(gap, EPS))


def build():
    fams = hc.families()
    cams = [pr.camera(f["K4"], f["dist"]) for f in fams]
    corners = np.stack([c for f in fams for c, _, _ in f["cases"]])
    fam = np.array([i for i, f in enumerate(fams) for _ in f["cases"]], np.int32)
    n = len(corners)
    valid = np.array([not fams[i]["degenerate"] for i in fam])
    z = lambda *s: np.full((n,) + s, np.nan)
    o = {"img": z(4, 2), "H": z(9), "kH": z(), "J": z(6), "Rst": z(2, 9), "rad_st": z(2), "k_rot": z(), "R": z(2, 9), "t": z(2, 3), "rms": z(2),
         "pimw": z(2), "rad": z(2), "F": z(2), "tst": z(2, 3), "kT": z(), "rp_err": np.full((n, 2), np.nan, np.float32), "S": z(6), "ev_h": z(3), "ev_gap": z(),
         "oracle_eR": z(2), "oracle_et": z(), "G": z(2)}
    W = {"H": 0.0, "rot": 0.0, "t": 0.0, "ev": 0.0}
    oracle_nan = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            f, cam = fams[fam[i]], cams[fam[i]]
            want = oracle_lib.marker_pose(corners[i], np.float32(f["size"]), f["K4"], f["dist"])
            flat = np.concatenate([np.concatenate(want[:4]), want[4]])
            oracle_nan[i] = np.isnan(flat).any()
            if not valid[i]:
                continue
            obj = pr.object_points(np.float32(f["size"]))
            s = pr.solve(MP, corners[i], np.float32(f["size"]), cam)
            o["img"][i] = s["img"]; o["H"][i] = tofloat(s["H"]); o["kH"][i] = pr.homography_condition(obj, s["img"])
            o["rad"][i] = tofloat(s["rad"])
            for k, sol in enumerate(s["sol"]):
                o["R"][i, k] = tofloat(sol["R"]); o["t"][i, k] = tofloat(sol["t"]); o["rms"][i, k] = float(sol["rms"])
                o["pimw"][i, k] = float(pr.mp.pi - sol["w"]); o["F"][i, k] = pr.rounding_change(sol["rvec"], sol["R"])
                o["G"][i, k] = 2 * np.sqrt(2) * max(cam["fx"], cam["fy"]) * f["size"] / abs(o["t"][i, k, 2])
            # the stages on double inputs: the reference of a stage is the 50-digit evaluation of exactly those doubles
            o["J"][i] = tofloat(s["J"])
            R1, R2, r0, r1 = pr.rotations(MP, o["J"][i])
            o["Rst"][i] = [tofloat(R1), tofloat(R2)]; o["rad_st"][i] = [float(r0), float(r1)]; o["k_rot"][i] = rot_condition(o["rad_st"][i])
            o["kT"][i] = pr.translation_condition(s["img"])
            for k in range(2):
                o["tst"][i, k] = tofloat(pr.translation(MP, obj, s["img"], o["R"][i, k]))
                o["rp_err"][i, k] = pr.reprojection_error_float(MP, obj, corners[i], cam, o["R"][i, k], o["t"][i, k])
            o["S"][i] = pr.ho_system(obj, s["img"])
            o["ev_h"][i], o["ev_gap"][i] = pr.smallest_eigenvector(o["S"][i])
            # the plain double evaluation of the same stages, in units of eps times the stage's condition
            Hd = np.array(pr.homography(F64, obj, s["img"]), np.float64)
            W["H"] = max(W["H"], np.abs(Hd - o["H"][i]).max() / (EPS * o["kH"][i] * np.abs(o["H"][i]).max()))
            if min(o["rad_st"][i]) > ZONE:
                Rd = pr.rotations(F64, o["J"][i])
                W["rot"] = max(W["rot"], max(np.abs(np.array(Rd[k], np.float64) - o["Rst"][i, k]).max() for k in range(2)) / (EPS * o["k_rot"][i]))
            for k in range(2):
                td = np.array(pr.translation(F64, obj, s["img"], o["R"][i, k]), np.float64)
                W["t"] = max(W["t"], np.abs(td - o["tst"][i, k]).max() / (EPS * o["kT"][i] * np.abs(o["tst"][i, k]).max()))
            lam, Q = np.linalg.eigh(np.array([[o["S"][i][0], o["S"][i][1], o["S"][i][2]], [o["S"][i][1], o["S"][i][3], o["S"][i][4]], [o["S"][i][2], o["S"][i][4], o["S"][i][5]]]))
            W["ev"] = max(W["ev"], eig_ratio(Q[:, 0], o["ev_h"][i], o["ev_gap"][i]))
            if not oracle_nan[i]:
                o["oracle_eR"][i], o["oracle_et"][i] = oracle_against(want, o["R"][i], o["t"][i])
        # a wider fronto-parallel sample for the envelope alone (the first records of each are the committed cases): eR (pi - w)^2 / eps
        # has a long tail there (median about 1), and the largest of 48 draws would not bound a second implementation's 48 draws
        env_eR, env_pimw = [], []
        for f, cam in zip(fams, cams):
            if f["fronto"]:
                for c, _, _ in hc.placed(ENVELOPE_N, f["seed"], 0.0, f["K4"], f["dist"])[len(f["cases"]):]:
                    want = oracle_lib.marker_pose(c, np.float32(f["size"]), f["K4"], f["dist"])
                    if np.isfinite(want[3]).all():
                        s = pr.solve(MP, c, np.float32(f["size"]), cam)
                        env_eR.append(oracle_against(want, np.array([tofloat(x["R"]) for x in s["sol"]]), np.array([tofloat(x["t"]) for x in s["sol"]]))[0])
                        env_pimw.append([float(pr.mp.pi - x["w"]) for x in s["sol"]])
        # the rot2vec stage set, and its plain double evaluation
        rvR, rv_pimw, rv_zero, rv_edge = rot2vec_stage_set()
        rv_eR = np.array([eR(np.array(pr.rot2vec(F64, m)[0], np.float64), m) for m in rvR])
        evx = psd_set()
        evx_ref = [pr.smallest_eigenvector(a) for a in evx]
        for a, (h, gap) in zip(evx, evx_ref):
            lam, Q = np.linalg.eigh(np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]]))
            W["ev"] = max(W["ev"], eig_ratio(Q[:, 0], h, gap))
        all_eR = np.concatenate([o["oracle_eR"][valid & ~oracle_nan].ravel(), np.ravel(env_eR), rv_eR[~rv_zero]])
        all_pimw = np.concatenate([o["pimw"][valid & ~oracle_nan].ravel(), np.ravel(env_pimw), rv_pimw[~rv_zero]])
        keep = np.isfinite(all_eR)          # a solution whose rot2vec gave NaN (see test_pose_ref_cpu.py) has no eR
        all_eR, all_pimw = all_eR[keep], all_pimw[keep]
        near = all_pimw < 1e-2
        A = float((all_eR[near] * all_pimw[near] ** 2 / EPS).max())
        B = float(all_eR[~near].max())
        rot_tol = lambda pimw: 4 * (A * EPS / pimw ** 2 + B)
        tolR = rot_tol(o["pimw"]) + o["F"]
        tolE = 1e-3 * (1 + o["rp_err"].astype(np.float64)) + o["G"] * rot_tol(o["pimw"])
        # two reprojection cases the solver never produces: theta = 0, and z = 0 (the identity puts all four corners there)
        nod = [i for i, f in enumerate(fams) if f["name"] == "fronto_nodist"][0]
        obj = pr.object_points(np.float32(hc.SIZE))
        rpx_t = np.array([[0.1, -0.05, 1.0], [0.01, 0.02, 0.0]])
        rpx_corners = np.array([[[300, 200], [340, 200], [340, 240], [300, 240]]] * 2, np.float32)
        rpx_err = np.array([pr.reprojection_error_float(MP, obj, rpx_corners[k], cams[nod], np.eye(3).ravel(), rpx_t[k]) for k in range(2)], np.float32)
        tolE = tolE.astype(np.float32)
        rv_tol = rot_tol(rv_pimw)
    assert np.isfinite(rpx_err).all()
    return {"corners": corners, "fam": fam, "valid": valid, "oracle_nan": oracle_nan,
            "fam_names": np.array([f["name"] for f in fams]), "fam_size": np.array([f["size"] for f in fams], np.float32),
            "fam_K4": np.stack([f["K4"] for f in fams]), "fam_ndist": np.array([len(f["dist"]) for f in fams], np.int32),
            "fam_dist": np.stack([np.concatenate([f["dist"], np.zeros(12 - len(f["dist"]), np.float32)]) for f in fams]),
            "fam_degenerate": np.array([f["degenerate"] for f in fams]), "fam_fronto": np.array([f["fronto"] for f in fams]),
            "cam17": np.stack([pr.camera17(c) for c in cams]),
            **{k: v for k, v in o.items() if k != "G"}, "tolR": tolR, "tolE": tolE,
            "A": np.float64(A), "B": np.float64(B), "W_H": np.float64(W["H"]), "W_rot": np.float64(W["rot"]), "W_t": np.float64(W["t"]), "W_ev": np.float64(W["ev"]),
            "rv_R": rvR, "rv_pimw": rv_pimw, "rv_zero": rv_zero, "rv_edge": rv_edge, "rv_tol": rv_tol,
            "evx": evx, "evx_h": np.stack([h for h, _ in evx_ref]), "evx_gap": np.array([g for _, g in evx_ref]),
            "rpx_cam": np.int32(nod), "rpx_t": rpx_t, "rpx_corners": rpx_corners, "rpx_err": rpx_err}


if __name__ == "__main__":
    import time
    t0 = time.time()
    d = build()
    np.savez_compressed(PATH, **d)
    print("%d cases, %d bytes, %.0f s; A = %.3g, B = %.3g, W_H = %.3g, W_rot = %.3g, W_t = %.3g, W_ev = %.3g; oracle NaN records %s" % (
        len(d["fam"]), os.path.getsize(PATH), time.time() - t0, d["A"], d["B"], d["W_H"], d["W_rot"], d["W_t"], d["W_ev"],
        {str(d["fam_names"][f]): int(d["oracle_nan"][d["fam"] == f].sum()) for f in np.unique(d["fam"][d["oracle_nan"]])}))
