"""The mock map of the GlobalBundleAdjustment shim (test infrastructure): the hand-built map of tests/lba_shim_map.py -- keyframes whose
order in memory is not their list order, a bad keyframe that sees some points, a bad map point, a bad marker, a marker observed from
a keyframe that is not handed over -- the files tests/gba_shim_driver.cpp reads, and the reference's collect step
(src/Optimizer.cc:76-232) restated in Python on that description."""
import numpy as np

import lba_cases as S
import lba_shim_map as L


def build(seed=31):
    """the map, and the keyframes handed to BundleAdjustment: all but the one at `left_out` (it sees marker 0 only), in mnId order"""
    m = L.build(seed)
    ids = [k["id"] for k in m["kfs"]]
    m["left_out"] = ids.index(3)
    m["order"] = [k for k in np.argsort(ids).tolist() if k != m["left_out"]]
    # one point loses every observer but the bad keyframe: it stays a point of the map and gets no edge
    bad = [k for k, f in enumerate(m["kfs"]) if f["bad"]][0]
    m["edgeless"] = [i for i, p in enumerate(m["mps"]) if bad in p["obs"] and not p["bad"]][0]
    m["mps"][m["edgeless"]]["obs"] = {bad: m["mps"][m["edgeless"]]["obs"][bad]}
    return m


def write(m, prefix):
    L.write(m, prefix)
    np.array(m["order"], np.int32).tofile(prefix + "_order.bin")


def collect(m, use_markers=True):
    """The reference's collect step on the description: (gba problem dict without its options, keyframes (memory positions), points,
    markers).  A std::map<KeyFrame*, ...> iterates in memory order = ascending position."""
    kfs, mps, mas = m["kfs"], m["mps"], m["mas"]
    vertices = [k for k in m["order"] if not kfs[k]["bad"]]
    index = {k: i for i, k in enumerate(vertices)}
    points = [i for i, p in enumerate(mps) if not p["bad"]]
    off, okf, oxy, ooct = [0], [], [], []
    for mp in points:
        for k in sorted(mps[mp]["obs"]):
            if kfs[k]["bad"] or k not in index:
                continue
            x, y, o = kfs[k]["kps"][mps[mp]["obs"][k]]
            okf.append(index[k]); oxy.append((x, y)); ooct.append(o)
        off.append(len(okf))
    markers = [a for a, ma in enumerate(mas) if not ma["bad"]] if use_markers else []
    moff, mkf, mcor = [0], [], []
    for ma in markers:
        for k in sorted(mas[ma]["obs"]):
            if kfs[k]["bad"] or k not in index:
                continue
            mkf.append(index[k]); mcor.append(kfs[k]["markers"][mas[ma]["obs"][k]][2])
        moff.append(len(mkf))
    pb = dict(Tcw=np.array([kfs[k]["T"] for k in vertices], np.float32), kf_fixed=np.array([1 if kfs[k]["id"] == 0 else 0 for k in vertices], np.uint8),
              x3Dw=np.array([mps[p]["X"] for p in points], np.float32), obs_offset=np.array(off, np.int32), obs_kf=np.array(okf, np.int32),
              obs_xy=np.array(oxy, np.float32).reshape(-1, 2), obs_octave=np.array(ooct, np.int32), K=m["K"], inv_level_sigma2=m["inv_level_sigma2"],
              Twm=np.array([mas[a]["Twm"] for a in markers], np.float32).reshape(-1, 3, 4),
              marker_local=np.repeat(S.marker_local()[None], len(markers), 0), mobs_offset=np.array(moff, np.int32),
              mobs_kf=np.array(mkf, np.int32), mobs_corners=np.array(mcor, np.float32).reshape(-1, 4, 2), marker_info=25.0,
              use_markers=1 if use_markers else 0)
    return pb, vertices, points, markers
