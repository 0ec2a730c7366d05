"""The contract of a marker pose record against the high-precision reference in tests/golden/pose_hard_cases.npz, as one function that
tests/test_pose_ref_cpu.py applies to the CPU oracle and tests/test_pose_gpu.py to the device.  numpy only.

For one record (rvec, tvec, rvec2, tvec2, err[2]) and its fixture row:
  NaN        none of the 14 values; or all of them, only where the record is degenerate or a reference radicand of computeRotations is
             within 64 eps of zero; or the rvec and the err of ONE solution (its tvec finite), only where that solution's reference
             rotation is within sqrt(64 eps) of a half turn: there 1 + 2 cos w = -1 + (pi - w)^2 rounds below -1 and rot2vec's acos
             has no value.  (The second way is what the oracle shows on fronto-parallel markers away from the optical axis.)
  tvec       the two solutions, as an unordered pair, within 1e-5 relative of the reference's
  eR         the largest entry of Rodrigues(rvec) - R_ref, at most tolR = 4 (A eps / (pi - w)^2 + B) + F of the fixture
  order      err[0] <= err[1]
  err        each equal to the float64 reprojection RMS of the record's own rvec and tvec within 1e-3 + 1e-3 err + G sqrt(3) 2^-24 |rvec|:
             self-consistent, so it holds whatever the conditioning, except for what rounding rvec to float does to the rotation --
             nothing up to a few turns, everything where rot2vec returns |rvec| = 4e7 for a rotation 2e-9 short of a half turn (the
             oracle does, fronto_nodist record 55).  G = 2 sqrt(2) max(fx, fy) size / |t_z| carries radians to pixels, as for tolE.
check() returns the NaN class of the record: "none", "all" or "solution"."""
import numpy as np

import pose_cases as pc
import pose_hard_cases as hc

EPS = 2.0 ** -52
ZONE = 64 * EPS
T_RTOL = 1e-5


class Fixture:
    def __init__(self, path):
        self.d = {k: v for k, v in np.load(path).items()}
        self.n = len(self.d["fam"])

    def __getitem__(self, k):
        return self.d[k]

    def camera(self, i):
        f = self.d["fam"][i]
        return self.d["fam_K4"][f], self.d["fam_dist"][f][:self.d["fam_ndist"][f]], float(self.d["fam_size"][f])

    def family(self, name):
        return np.flatnonzero(self.d["fam"] == list(self.d["fam_names"]).index(name))


def reprojection_rms(rvec, tvec, corners, size, K4, dist):
    c = hc.project12(pc.object_points(size), pc.rodrigues(np.asarray(rvec, np.float64)), np.asarray(tvec, np.float64), K4, dist)
    return float(np.sqrt(((c - np.asarray(corners, np.float64)) ** 2).sum() / 8))


def e_rot(rvec, R):
    return float(np.abs(pc.rodrigues(np.asarray(rvec, np.float64)) - np.asarray(R, np.float64).reshape(3, 3)).max())


def check(fx, i, rvec, tvec, rvec2, tvec2, err, who=""):
    """asserts the contract for record i; -> (NaN class, [eR per reference solution or nan])"""
    rv = np.array([rvec, rvec2], np.float64); tv = np.array([tvec, tvec2], np.float64); err = np.asarray(err, np.float64)
    K4, dist, size = fx.camera(i)
    tag = (who, i, str(fx["fam_names"][fx["fam"][i]]))
    nan = np.concatenate([np.isnan(rv[0]), np.isnan(tv[0]), np.isnan(rv[1]), np.isnan(tv[1]), np.isnan(err)])
    if nan.all():
        assert not fx["valid"][i] or fx["rad"][i].min() <= ZONE, tag + ("all NaN away from a zero radicand", fx["rad"][i])
        return "all", [np.nan, np.nan]
    if not fx["valid"][i]:
        assert not nan.any(), tag + ("a degenerate record partly NaN", rv, tv, err)
        return "none", [np.nan, np.nan]
    assert not np.isnan(tv).any(), tag + ("NaN translation in a record that is not all NaN", tv)
    lost = [bool(np.isnan(rv[k]).any() or np.isnan(err[k])) for k in range(2)]
    for k in range(2):
        assert not lost[k] or (np.isnan(rv[k]).all() and np.isnan(err[k])), tag + ("a solution partly NaN", rv[k], err[k])
    assert not all(lost), tag + ("both rotation vectors NaN with finite translations", rv, err)
    R, t, tolR, pimw = fx["R"][i], fx["t"][i], fx["tolR"][i], fx["pimw"][i]
    failures = []
    for order in ((0, 1), (1, 0)):          # which reference solution each of the record's two is held to
        bad = []
        for k, r in enumerate(order):
            rel = np.abs(tv[k] - t[r]).max() / np.abs(t[r]).max()
            if rel > T_RTOL:
                bad.append(("tvec", k, r, rel))
            if lost[k]:
                if pimw[r] ** 2 > ZONE:
                    bad.append(("NaN rotation vector away from a half turn", k, r, pimw[r]))
            elif e_rot(rv[k], R[r]) > tolR[r]:
                bad.append(("eR", k, r, e_rot(rv[k], R[r]), tolR[r], pimw[r]))
        if not bad:
            eR = [np.nan, np.nan]
            for k, r in enumerate(order):
                eR[r] = np.nan if lost[k] else e_rot(rv[k], R[r])
            break
        failures.append(bad)
    else:
        raise AssertionError(tag + (failures, rv, tv, err))
    if not any(lost):
        assert err[0] <= err[1], tag + ("order", err)
    for k in range(2):
        if not lost[k]:
            rms = reprojection_rms(rv[k], tv[k], fx["corners"][i], size, K4, dist)
            G = 2 * np.sqrt(2) * float(max(K4[:2])) * size / abs(tv[k][2])
            tol = 1e-3 + 1e-3 * err[k] + G * np.sqrt(3) * 2.0 ** -24 * np.linalg.norm(rv[k])
            assert abs(err[k] - rms) <= tol, tag + ("err against its own pose", k, err[k], rms, tol)
    return ("solution" if any(lost) else "none"), eR


def nan_class(rec14):
    """the NaN pattern of records n x 14 (rvec tvec rvec2 tvec2 err[2]) without a reference: 0 none, 1 all, 2 one solution's rvec and err,
    -1 anything else"""
    nan = np.isnan(np.asarray(rec14).reshape(-1, 14))
    sol = [np.array([0, 1, 2, 12]), np.array([6, 7, 8, 13])]
    out = np.full(len(nan), -1)
    out[~nan.any(1)] = 0
    out[nan.all(1)] = 1
    for s in sol:
        only = nan[:, s].all(1) & (nan.sum(1) == 4)
        out[only] = 2
    return out


def flat14(p):
    """binding.POSE_DTYPE records -> n x 14"""
    return np.concatenate([p["rvec"], p["tvec"], p["rvec2"], p["tvec2"], p["err"]], axis=1).astype(np.float32)
