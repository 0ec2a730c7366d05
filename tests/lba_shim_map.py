"""A hand-built mock map for the LocalBundleAdjustment shim (test infrastructure): a scene of tests/lba_cases.py turned into keyframes,
map points and map markers the way ORB_SLAM2 holds them, with the things the collect step has to get right -- keyframes whose order
in memory (the order of every std::map<KeyFrame*, ...>) is not their list order, a bad covisible keyframe, a bad map point, an old
marker entry, a marker seen from two keyframes (one id, one vertex), a marker observation from a keyframe that is no vertex, the
mnId 0 keyframe among the local ones -- the files the driver tests/lba_shim_driver.cpp reads, and the reference's collect step
(src/Optimizer.cc:777-1115) restated in Python on that description."""
import numpy as np

import lba_cases as S

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def build(seed=31):
    pb = S.scene(3, 2, 90, seed, out_frac=0.08, markers=((1, 2, 4), (2, 3)))
    rng = np.random.RandomState(seed)
    nflat = len(pb["Tcw"])                        # flat order: mnId 0 keyframe, 3 free local ones, 2 fixed cameras
    # two more keyframes: a bad covisible one (slot 6) and one that sees marker 0 only and is no vertex (slot 7)
    T = np.concatenate([pb["Tcw"].reshape(-1, 3, 4), pb["Tcw"].reshape(-1, 3, 4)[[1, 2]]])
    nk = len(T)
    place = rng.permutation(nk)                   # place[flat index] = position in memory
    kfs = [None] * nk
    ids = [0, 11, 12, 13, 5, 7, 14, 3]            # mnId
    for f in range(nk):
        kfs[place[f]] = dict(id=ids[f], bad=(f == 6), T=T[f], kps=[], matches=[], markers=[])
    mps = []
    for i in range(len(pb["x3Dw"])):
        obs = {}
        for e in range(pb["obs_offset"][i], pb["obs_offset"][i + 1]):
            k = place[pb["obs_kf"][e]]
            feat = len(kfs[k]["kps"])
            kfs[k]["kps"].append((pb["obs_xy"][e, 0], pb["obs_xy"][e, 1], int(pb["obs_octave"][e])))
            kfs[k]["matches"].append(i)
            obs[int(k)] = feat
        if i % 9 == 0:                            # the bad covisible keyframe sees some points too: its edges are skipped
            k = place[6]
            obs[int(k)] = len(kfs[k]["kps"])
            kfs[k]["kps"].append((100.0 + i, 80.0, 0))
            kfs[k]["matches"].append(i)
        mps.append(dict(X=pb["x3Dw"][i], bad=(i == 17), obs=obs))
    mas = [dict(id=40, bad=False, Twm=pb["Twm"].reshape(-1, 3, 4)[0], obs={}), dict(id=41, bad=False, Twm=pb["Twm"].reshape(-1, 3, 4)[1], obs={}),
           dict(id=42, bad=True, Twm=pb["Twm"].reshape(-1, 3, 4)[1], obs={})]
    for m in range(2):
        for o in range(pb["mobs_offset"][m], pb["mobs_offset"][m + 1]):
            k = place[pb["mobs_kf"][o]]
            mas[m]["obs"][int(k)] = len(kfs[k]["markers"])
            kfs[k]["markers"].append((m, False, pb["mobs_corners"].reshape(-1, 4, 2)[o]))
    k = place[7]                                  # not a vertex: its observation of marker 0 is left out
    mas[0]["obs"][int(k)] = 0
    kfs[k]["markers"].append((0, False, pb["mobs_corners"].reshape(-1, 4, 2)[0] + 1))
    k = place[2]                                  # an old entry and a bad marker in a local keyframe: neither makes a vertex
    kfs[k]["markers"].append((1, True, pb["mobs_corners"].reshape(-1, 4, 2)[0]))
    kfs[k]["markers"].append((2, False, pb["mobs_corners"].reshape(-1, 4, 2)[0]))
    cur = int(place[2])
    cov = [int(place[f]) for f in (3, 6, 0, 1)]   # by weight; the bad one in the middle
    return dict(kfs=kfs, mps=mps, mas=mas, cur=cur, cov=cov, K=pb["K"], inv_level_sigma2=pb["inv_level_sigma2"], side=S.MARKER_SIDE)


def write(m, prefix):
    kfs, mps, mas = m["kfs"], m["mps"], m["mas"]
    np.array([[k["id"], k["bad"], len(k["kps"]), len(k["markers"])] for k in kfs], np.int32).tofile(prefix + "_kf.bin")
    np.array([k["T"] for k in kfs], np.float32).tofile(prefix + "_kfT.bin")
    kp = np.zeros(sum(len(k["kps"]) for k in kfs), KP)
    match = np.zeros(len(kp), np.int32)
    j = 0
    for k in kfs:
        for (x, y, o), mp in zip(k["kps"], k["matches"]):
            kp[j]["x"], kp[j]["y"], kp[j]["octave"] = x, y, o
            match[j] = mp
            j += 1
    kp.tofile(prefix + "_kps.bin"); match.tofile(prefix + "_match.bin")
    np.array([(mk[0], mk[1]) for k in kfs for mk in k["markers"]], np.int32).reshape(-1, 2).tofile(prefix + "_kfmk.bin")
    np.array([mk[2] for k in kfs for mk in k["markers"]], np.float32).tofile(prefix + "_kfcorners.bin")
    np.array([p["X"] for p in mps], np.float32).tofile(prefix + "_X.bin")
    np.array([p["bad"] for p in mps], np.uint8).tofile(prefix + "_mpbad.bin")
    np.array([(i, k, f) for i, p in enumerate(mps) for k, f in sorted(p["obs"].items())], np.int32).reshape(-1, 3).tofile(prefix + "_obs.bin")
    np.array([(a["id"], a["bad"]) for a in mas], np.int32).tofile(prefix + "_ma.bin")
    np.array([a["Twm"] for a in mas], np.float32).tofile(prefix + "_maT.bin")
    np.array([(i, k, s) for i, a in enumerate(mas) for k, s in sorted(a["obs"].items())], np.int32).reshape(-1, 3).tofile(prefix + "_maobs.bin")
    np.array([m["cur"]] + m["cov"], np.int32).tofile(prefix + "_cur.bin")
    np.concatenate([np.asarray(m["K"], np.float32).reshape(4), [m["side"]], m["inv_level_sigma2"]]).astype(np.float32).tofile(prefix + "_cam.bin")


def collect(m, use_markers=True):
    """The reference's collect step on the description: (lba problem dict, vertex keyframes (memory positions), nlocal, points, markers,
    edges [(keyframe position, point)]).  A std::map<KeyFrame*, ...> iterates in memory order = ascending position."""
    kfs, mps, mas = m["kfs"], m["mps"], m["mas"]
    local = [m["cur"]] + [k for k in m["cov"] if not kfs[k]["bad"]]
    marked_local = set([m["cur"]] + m["cov"])
    points = []
    for k in local:
        for mp in kfs[k]["matches"]:
            if not mps[mp]["bad"] and mp not in points:
                points.append(mp)
    fixed, marked_fixed = [], set()
    for mp in points:
        for k in sorted(mps[mp]["obs"]):
            if k not in marked_local and k not in marked_fixed:
                marked_fixed.add(k)
                if not kfs[k]["bad"]:
                    fixed.append(k)
    markers, seen_ids = [], []
    for k in local + fixed:
        for (ma, old, _) in kfs[k]["markers"]:
            if old or mas[ma]["bad"] or mas[ma]["id"] in seen_ids:
                continue
            markers.append(ma)
            seen_ids.append(mas[ma]["id"])
    vertices = local + fixed
    index = {k: i for i, k in enumerate(vertices)}
    off, okf, oxy, ooct, edges = [0], [], [], [], []
    for mp in points:
        for k in sorted(mps[mp]["obs"]):
            if kfs[k]["bad"]:
                continue
            x, y, o = kfs[k]["kps"][mps[mp]["obs"][k]]
            okf.append(index[k]); oxy.append((x, y)); ooct.append(o); edges.append((k, mp))
        off.append(len(okf))
    moff, mkf, mcor = [0], [], []
    for ma in markers:
        for k in sorted(mas[ma]["obs"]):
            if kfs[k]["bad"] or k not in index:
                continue
            mkf.append(index[k]); mcor.append(kfs[k]["markers"][mas[ma]["obs"][k]][2])
        moff.append(len(mkf))
    pb = dict(Tcw=np.array([kfs[k]["T"] for k in vertices], np.float32), kf_fixed=np.array([1 if (i >= len(local) or kfs[k]["id"] == 0) else 0 for i, k in enumerate(vertices)], np.uint8),
              x3Dw=np.array([mps[p]["X"] for p in points], np.float32), obs_offset=np.array(off, np.int32), obs_kf=np.array(okf, np.int32),
              obs_xy=np.array(oxy, np.float32).reshape(-1, 2), obs_octave=np.array(ooct, np.int32), K=m["K"], inv_level_sigma2=m["inv_level_sigma2"],
              Twm=np.array([mas[a]["Twm"] for a in markers], np.float32).reshape(-1, 3, 4),
              marker_local=np.repeat(S.marker_local()[None], len(markers), 0), mobs_offset=np.array(moff, np.int32),
              mobs_kf=np.array(mkf, np.int32), mobs_corners=np.array(mcor, np.float32).reshape(-1, 4, 2), marker_info=25.0,
              use_markers=1 if use_markers else 0)
    return pb, vertices, len(local), points, markers, edges
