"""Seeded synthetic GlobalBundleAdjustment problems (test infrastructure): keyframes along an arc or a ring looking at a point cloud,
every point seen from a short run of consecutive keyframes (or from all of them), float observations at octave-scaled noise, gross
outliers where marked, markers at known poses, perturbed initial poses and points.  A case is a dict binding.gba_arrays takes
(iterations, robust and leaf_vertices included), plus the ground truth ("true": Tcw, x3Dw, Twm).  The named cases are the smallest
shapes that reach each mechanism of the solver, not the workload."""
import numpy as np

from lba_cases import INV_SIGMA2, K4, NLEVELS, RADIUS, extent, look_at, marker_local, project, rodrigues  # noqa: F401


def track(nkf, npts, seed, span=(3, 5), ring=False, fixed=(0,), markers=(), out_frac=0.0, noise=0.5, all_see=False, arc=2.0, perturb=1.0):
    """nkf keyframes in temporal order on an arc of `arc` radians (ring: the full circle, first and last covisible); point i is seen
    from span[0] .. span[1] consecutive keyframes (all_see: from every one).  markers: one tuple of observing keyframes per marker."""
    rng = np.random.RandomState(seed)
    ang = np.arange(nkf) * (2 * np.pi / nkf) if ring else (np.linspace(-arc / 2, arc / 2, nkf) if nkf > 1 else np.zeros(1))
    T = np.zeros((nkf, 3, 4))
    for k in range(nkf):
        T[k] = look_at(np.array([RADIUS * np.sin(ang[k]), 0.3 * np.cos(3 * ang[k]), -RADIUS * np.cos(ang[k])]))
    kf_fixed = np.zeros(nkf, np.uint8)
    kf_fixed[list(fixed)] = 1
    X = rng.normal(0, 0.6, (npts, 3))
    off, okf, oxy, ooct, outl = [0], [], [], [], []
    for i in range(npts):
        if all_see:
            see = np.arange(nkf)
        else:
            n = int(rng.randint(span[0], span[1] + 1))
            s = int(rng.randint(0, nkf if ring else nkf - n + 1))
            see = (s + np.arange(n)) % nkf
        see = see[rng.permutation(len(see))]   # GetObservations() is ordered by pointer, not by keyframe index
        for k in see:
            uv, _ = project(T[k], X[i:i + 1])
            o = int(rng.randint(0, 4))
            bad = rng.rand() < out_frac
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

    pb = dict(Tcw=shake(T, kf_fixed == 0, 0.01, 0.03).astype(np.float32), kf_fixed=kf_fixed,
              x3Dw=(X + rng.normal(0, 0.03 * perturb, X.shape)).astype(np.float32), obs_offset=np.array(off, np.int32),
              obs_kf=np.array(okf, np.int32), obs_xy=np.array(oxy, np.float32).reshape(-1, 2), obs_octave=np.array(ooct, np.int32),
              K=K4.copy(), inv_level_sigma2=INV_SIGMA2.copy(),
              Twm=shake(Twm, np.ones(len(markers), bool), 0.01, 0.01).astype(np.float32),
              marker_local=np.repeat(loc[None], len(markers), 0).astype(np.float32), mobs_offset=np.array(moff, np.int32),
              mobs_kf=np.array(mkf, np.int32), mobs_corners=np.array(mcor, np.float32).reshape(-1, 4, 2), marker_info=25.0,
              use_markers=1 if markers else 0, outlier=np.array(outl, bool), iterations=10, robust=0, leaf_vertices=0,
              true=dict(Tcw=T, x3Dw=X, Twm=Twm))
    pb["Tcw"][kf_fixed != 0] = T[kf_fixed != 0].astype(np.float32)
    return pb


def _drop(pb, keep):
    """pb without the observation slots where keep is False"""
    cnt = np.add.reduceat(keep.astype(np.int64), pb["obs_offset"][:-1]) * (np.diff(pb["obs_offset"]) > 0)
    for key in ("obs_kf", "obs_xy", "obs_octave", "outlier"):
        pb[key] = pb[key][keep]
    pb["obs_offset"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    return pb


def _orphans(noise=0.5, seed=31):
    """point 5 without observations, free keyframe 3 without an edge, marker 1 without observations"""
    pb = track(7, 150, seed, markers=((0, 1, 2), ()), noise=noise)
    keep = pb["obs_kf"] != 3
    keep[pb["obs_offset"][5]:pb["obs_offset"][6]] = False
    _drop(pb, keep)
    assert pb["obs_offset"][6] == pb["obs_offset"][5] and (np.diff(pb["obs_offset"]) > 0).sum() == 149
    pb["lonely_point"], pb["lonely_keyframe"], pb["lonely_marker"] = 5, 3, 1
    return pb


def _z0(noise=0.5, seed=33):
    """observation 0's point lies in the plane z = 0 of its keyframe, exactly: an identity pose and a point with z = 0.  That keyframe
    is made a fixed camera that sees this one point only, so the rest of the problem stays sound."""
    pb = track(5, 80, seed, noise=noise)
    k = int(pb["obs_kf"][0])
    pb["Tcw"][k] = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    pb["x3Dw"][0] = (0.3, -0.2, 0.0)
    keep = pb["obs_kf"] != k
    keep[0] = True
    _drop(pb, keep)
    pb["kf_fixed"][k] = 1
    pb["z0_slot"] = 0
    return pb


# the shapes, as functions of the pixel noise (the CPU tests run them noise-free too)
SHAPES = {
    "init2_p120": lambda noise: track(2, 120, 41, all_see=True, arc=0.35, noise=noise),
    "init2_p120_m1": lambda noise: track(2, 120, 42, all_see=True, arc=0.35, markers=((0, 1),), noise=noise),
    "chain12_p400": lambda noise: track(12, 400, 43, noise=noise),
    "ring24_p600_m3_out": lambda noise: track(24, 600, 44, ring=True, markers=((0, 1, 2), (11, 12, 13), (3, 4, 15, 16)), out_frac=0.10 if noise else 0.0,
                                              noise=noise),
    "dense8_p200": lambda noise: track(8, 200, 45, all_see=True, arc=1.4, noise=noise),
    "k70_p300": lambda noise: track(71, 300, 46, arc=2.6, noise=noise),
    "nofixed6_p150": lambda noise: track(6, 150, 47, fixed=(), arc=1.2, noise=noise),
    "orphans": _orphans,
    "obs64_p12": lambda noise: track(64, 12, 48, all_see=True, arc=2.2, noise=noise),
    "z0": _z0,
    "p257": lambda noise: track(3, 257, 49, all_see=True, arc=0.6, noise=noise),
}

# the runs: a shape with its options.  10 iterations without Huber is the loop-closing call, 20 with it the initial-map call.
CASES = {
    "init2_p120_r20": ("init2_p120", dict(iterations=20, robust=1)),
    "init2_p120_m1_r0": ("init2_p120_m1", dict(iterations=20, robust=0)),
    "init2_p120_m1_r1": ("init2_p120_m1", dict(iterations=20, robust=1)),
    "chain12_p400_leaf2": ("chain12_p400", dict(leaf_vertices=2)),
    "chain12_p400": ("chain12_p400", dict()),
    "ring24_p600_m3_out_r1": ("ring24_p600_m3_out", dict(robust=1, leaf_vertices=2)),
    "ring24_p600_m3_out_r0": ("ring24_p600_m3_out", dict(robust=0, leaf_vertices=2)),
    "dense8_p200": ("dense8_p200", dict()),
    "k70_p300": ("k70_p300", dict()),
    "nofixed6_p150": ("nofixed6_p150", dict()),
    "orphans": ("orphans", dict(leaf_vertices=2)),
    "orphans_markers_unused": ("orphans", dict(use_markers=0)),
    "obs64_p12": ("obs64_p12", dict()),
    "z0": ("z0", dict(robust=1)),
    "p257": ("p257", dict(robust=1)),
}


def case(name, noise=0.5):
    shape, opts = CASES[name]
    return dict(SHAPES[shape](noise), **opts)


def chain(nkf, npts, seed=50):
    """a chain of any length, for the plan's scaling check"""
    return track(nkf, npts, seed)


def complete_graph(nkf):
    """nkf keyframes that all see one point: a complete covisibility graph (the plan alone looks at it: the point is past the
    observation bound of the calls)"""
    return track(nkf, 1, 51, all_see=True)


def bad_octave():
    pb = case("init2_p120_r20")
    pb["obs_octave"] = pb["obs_octave"].copy()
    pb["obs_octave"][17] = NLEVELS
    return pb


def obs257():
    return track(257, 3, 52, all_see=True)
