"""Seeded synthetic LocalBundleAdjustment problems (test infrastructure): keyframes on an arc looking at a point cloud, float
observations at octave-scaled noise, gross outliers, markers at known poses, perturbed initial poses and points.  A case is a dict
binding.lba_arrays takes, plus the ground truth ("true": Tcw, x3Dw, Twm) and "outlier" (a flag per observation slot).  The named
cases are the smallest at which each mechanism of the solver can go wrong, not the workload."""
import numpy as np

K4 = np.array([520.0, 515.0, 322.5, 238.5], np.float32)
NLEVELS = 8
INV_SIGMA2 = (1.0 / 1.2 ** (2 * np.arange(NLEVELS))).astype(np.float32)
MARKER_SIDE = 0.25
RADIUS = 4.0


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def look_at(center, target=np.zeros(3)):
    z = target - center
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                    # rows: camera axes in the world
    return np.hstack([R, (-R @ center)[:, None]])


def project(T, X):
    Xc = X @ T[:, :3].T + T[:, 3]
    return np.stack([Xc[:, 0] / Xc[:, 2] * K4[0] + K4[2], Xc[:, 1] / Xc[:, 2] * K4[1] + K4[3]], 1), Xc[:, 2]


def marker_local():
    s = MARKER_SIDE / 2
    return np.array([[-s, s, 0], [s, s, 0], [s, -s, 0], [-s, -s, 0]], np.float32)


def scene(nfree, nfixed, npts, seed, first_fixed=True, out_frac=0.0, noise=0.5, vis=0.6, markers=(), perturb=1.0, all_see=False,
          arc=1.2, min_obs=2, one_outlier_a_point=False):
    """nfree free keyframes (the first of the list is the mnId 0 keyframe when first_fixed: fixed, but a local one), then nfixed fixed
    cameras.  markers: one tuple of observing keyframe indices per marker."""
    rng = np.random.RandomState(seed)
    nloc = nfree + (1 if first_fixed else 0)
    nkf = nloc + nfixed
    ang = np.linspace(-arc / 2, arc / 2, nkf) if nkf > 1 else np.zeros(1)
    order = rng.permutation(nkf)               # local and fixed keyframes interleave along the arc
    T = np.zeros((nkf, 3, 4))
    for k in range(nkf):
        a = ang[order[k]]
        T[k] = look_at(np.array([RADIUS * np.sin(a), 0.3 * np.cos(3 * a), -RADIUS * np.cos(a)]))
    fixed = np.zeros(nkf, np.uint8)
    fixed[nloc:] = 1
    if first_fixed:
        fixed[0] = 1
    X = rng.normal(0, 0.6, (npts, 3))
    off, okf, oxy, ooct, outl = [0], [], [], [], []
    for i in range(npts):
        see = np.arange(nkf) if all_see else np.nonzero(rng.rand(nkf) < vis)[0]
        if len(see) < min_obs:
            see = rng.choice(nkf, min(min_obs, nkf), replace=False)
        see = see[rng.permutation(len(see))]   # GetObservations() is ordered by pointer, not by keyframe index
        for k in see:
            uv, _ = project(T[k], X[i:i + 1])
            o = int(rng.randint(0, 4))
            bad = rng.rand() < out_frac
            if one_outlier_a_point and any(outl[off[-1]:]):
                bad = False
            uv = uv[0] + rng.normal(0, noise * 1.2 ** o, 2) + (rng.choice([-1, 1], 2) * rng.uniform(15, 60, 2) if bad else 0)
            okf.append(k); oxy.append(uv); ooct.append(o); outl.append(bad)
        off.append(len(okf))
    Twm = np.zeros((len(markers), 3, 4))
    moff, mkf, mcor = [0], [], []
    loc = marker_local()
    for m, seen_by in enumerate(markers):
        Twm[m, :, :3] = rodrigues(rng.normal(0, 0.3, 3))
        Twm[m, :, 3] = rng.normal(0, 0.5, 3)
        Pw = loc.astype(np.float64) @ Twm[m, :, :3].T + Twm[m, :, 3]
        for k in seen_by:
            uv, _ = project(T[k], Pw)
            mkf.append(k); mcor.append(uv + rng.normal(0, 0.4 * noise, (4, 2)))
        moff.append(len(mkf))

    def shake(Ts, mask, rs, ts):
        out = Ts.copy()
        for k in np.nonzero(mask)[0]:
            dR = rodrigues(rng.normal(0, rs * perturb, 3))
            out[k, :, :3] = dR @ Ts[k, :, :3]
            out[k, :, 3] = dR @ Ts[k, :, 3] + rng.normal(0, ts * perturb, 3)
        return out

    pb = dict(Tcw=shake(T, fixed == 0, 0.01, 0.03).astype(np.float32), kf_fixed=fixed,
              x3Dw=(X + rng.normal(0, 0.03 * perturb, X.shape)).astype(np.float32), obs_offset=np.array(off, np.int32),
              obs_kf=np.array(okf, np.int32), obs_xy=np.array(oxy, np.float32).reshape(-1, 2), obs_octave=np.array(ooct, np.int32),
              K=K4.copy(), inv_level_sigma2=INV_SIGMA2.copy(),
              Twm=shake(Twm, np.ones(len(markers), bool), 0.01, 0.01).astype(np.float32),
              marker_local=np.repeat(loc[None], len(markers), 0).astype(np.float32), mobs_offset=np.array(moff, np.int32),
              mobs_kf=np.array(mkf, np.int32), mobs_corners=np.array(mcor, np.float32).reshape(-1, 4, 2), marker_info=25.0,
              use_markers=1 if markers else 0, outlier=np.array(outl, bool),
              true=dict(Tcw=T, x3Dw=X, Twm=Twm))
    # the fixed keyframes hold their true poses, rounded to float as the map holds them
    pb["Tcw"][fixed != 0] = T[fixed != 0].astype(np.float32)
    return pb


def extent(pb):
    return float(np.ptp(pb["true"]["x3Dw"], 0).max()) if len(pb["true"]["x3Dw"]) else 1.0


def _k4f2(seed=2):
    """fixed cameras present; the last 40 points are seen by the two fixed cameras and exactly one free keyframe"""
    pb = scene(4, 2, 300, seed, first_fixed=False, out_frac=0.10)
    rng = np.random.RandomState(seed + 1000)
    T, X = pb["true"]["Tcw"], pb["true"]["x3Dw"]
    keep = pb["obs_offset"][260]
    okf, oxy, ooct, outl, off = list(pb["obs_kf"][:keep]), list(pb["obs_xy"][:keep]), list(pb["obs_octave"][:keep]), list(pb["outlier"][:keep]), list(pb["obs_offset"][:261])
    for i in range(260, 300):
        for k in (4, int(rng.randint(0, 4)), 5):
            uv, _ = project(T[k], X[i:i + 1])
            okf.append(k); oxy.append(uv[0] + rng.normal(0, 0.5, 2)); ooct.append(0); outl.append(False)
        off.append(len(okf))
    pb.update(obs_kf=np.array(okf, np.int32), obs_xy=np.array(oxy, np.float32), obs_octave=np.array(ooct, np.int32), outlier=np.array(outl, bool),
              obs_offset=np.array(off, np.int32))
    return pb


def _special(seed=5):
    """a point with a single observation, a free keyframe without observations, a marker all of whose edges go to level 1"""
    pb = scene(4, 2, 120, seed, out_frac=0.05, markers=((0, 1, 5), (1, 2)))
    lonely = 3                                      # free keyframe 3 loses every observation
    keep = pb["obs_kf"] != lonely
    cnt = np.add.reduceat(keep.astype(np.int64), pb["obs_offset"][:-1])
    # point 7 keeps one observation only
    lo, hi = pb["obs_offset"][7], pb["obs_offset"][8]
    first = lo + int(np.argmax(keep[lo:hi]))
    keep[lo:hi] = False
    keep[first] = True
    cnt[7] = 1
    assert cnt.min() >= 1
    for k in ("obs_kf", "obs_xy", "obs_octave", "outlier"):
        pb[k] = pb[k][keep]
    pb["obs_offset"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    # marker 1: every corner observation 40 px off, in different directions per keyframe, so no pose explains them
    lo, hi = pb["mobs_offset"][1], pb["mobs_offset"][2]
    for j, o in enumerate(range(lo, hi)):
        pb["mobs_corners"][o] += np.array([[40, -35], [-38, 42], [36, 39], [-41, -37]], np.float32) * (1 if j % 2 == 0 else -1)
    pb["lonely_keyframe"], pb["single_point"], pb["dead_marker"] = lonely, 7, 1
    return pb


def _full_obs(nkf, npts, seed):
    """every point is seen by every one of nkf keyframes (4 free, the mnId 0 one, the rest fixed cameras)"""
    return scene(4, nkf - 5, npts, seed, all_see=True, arc=2.0)


def _markers_only(seed=8):
    pb = scene(3, 1, 0, seed, markers=((0, 1, 4), (1, 2, 3, 4)))
    return pb


def _z0(seed=9):
    """observation 0's point lies in the plane z = 0 of its keyframe, exactly: an identity pose and a point with z = 0"""
    pb = scene(3, 1, 60, seed)
    k = int(pb["obs_kf"][0])
    pb["Tcw"][k] = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    pb["x3Dw"][0] = (0.3, -0.2, 0.0)
    # that keyframe now looks elsewhere: it is made a fixed camera that sees this one point only, so the rest of the problem stays sound
    keep = (pb["obs_kf"] != k)
    keep[0] = True
    cnt = np.add.reduceat(keep.astype(np.int64), pb["obs_offset"][:-1])
    for key in ("obs_kf", "obs_xy", "obs_octave", "outlier"):
        pb[key] = pb[key][keep]
    pb["obs_offset"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    pb["kf_fixed"][k] = 1
    pb["z0_slot"] = 0
    return pb


def _bound(nfree, seed=10):
    """nfree free keyframes (and the mnId 0 one), few points: the pose bound"""
    return scene(nfree, 0, 150, seed, vis=0.15, arc=2.4)


CASES = {
    "k3_p40_clean": lambda: scene(2, 0, 40, 1, noise=0.0),
    "k3_p40_clean_m1": lambda: scene(2, 0, 40, 11, noise=0.0, markers=((0, 1, 2),)),
    "k4f2_p300_out10": _k4f2,
    "k6f3_p1000_out20_m2": lambda: scene(6, 3, 1000, 3, first_fixed=False, out_frac=0.20, markers=((0, 7), (1, 2, 4))),
    # every injected outlier is decidable: at least five observations a point, at most one of them an outlier
    "k6f3_p250_out8_decidable": lambda: scene(6, 3, 250, 16, first_fixed=False, out_frac=0.08, vis=0.75, min_obs=5, one_outlier_a_point=True),
    "k3_p257": lambda: scene(2, 0, 257, 4, out_frac=0.05),
    "k256_p12_obs256": lambda: _full_obs(256, 12, 6),     # ORBFE_LBA_MAX_OBSERVATIONS observations a point, exactly
    "k64_p70_obs64": lambda: _full_obs(64, 70, 7),        # 64 observations a point: one wave's worth; two workgroups of points
    "special": _special,
    "markers_given_unused": lambda: dict(scene(3, 1, 80, 12, out_frac=0.05, markers=((0, 1), (2, 3))), use_markers=0),
    "no_markers": lambda: scene(3, 2, 80, 13, out_frac=0.05),
    "np0_markers_only": _markers_only,
    "free64": lambda: _bound(64),
    "z0": _z0,
}


def restarted(pb, times=1):
    """pb with the restatement's own result as the initial estimates: a problem that starts converged, so that the first round's
    trials are rejected down to rounding"""
    import lba_build
    for _ in range(times):
        r = lba_build.local_bundle_adjustment(pb, lba_build.INSERTION)
        pb = dict(pb, Tcw=r["Tcw"].copy(), x3Dw=r["x3Dw"].copy(), Twm=r["Twm"].copy())
    return pb


def golden(name):
    """a recorded problem of tests/golden/: the parity input does not depend on a run of the code under comparison"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    pb = {k: z[k] for k in z.files if not k.startswith("true_")}
    pb.update(marker_info=25.0, use_markers=0, true=dict(Tcw=z["true_Tcw"], x3Dw=z["true_x3Dw"], Twm=z["true_Twm"]))
    return pb


# found by seed search on the CPU restatement (tests/test_lba_cpu.py checks that they still do): rounds that end on a rejected trial.
# No seed of some 1 500 fresh scenes ended round 1 that way (five iterations do not converge far enough); restarted ones do.
STALE_CASES = {
    "stale_r1": lambda: golden("lba_stale_r1"),                           # stale_mask 3: restarted(scene(3, 1, 60, 306), 1), recorded
    "stale_r2": lambda: scene(2, 0, 40, 103, perturb=3.0),                # stale_mask 2
}


def case(name):
    return (CASES.get(name) or STALE_CASES[name])()


def over_bound():
    return _bound(65)


def obs257():
    return _full_obs(257, 3, 14)


def bad_octave():
    pb = scene(2, 0, 40, 15)
    pb["obs_octave"] = pb["obs_octave"].copy()
    pb["obs_octave"][17] = NLEVELS
    return pb


def timing_problem(seed=21):
    """local-mapping sized: 20 free + 20 fixed keyframes, 3 000 points, 2 markers, 10 % outliers"""
    return scene(20, 20, 3000, seed, first_fixed=False, out_frac=0.10, vis=0.35, markers=((0, 3, 25), (5, 6, 7, 30)))
