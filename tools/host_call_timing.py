"""Host-clock medians of the host-pointer calls that stage through a thread's host stage: orbfe_knn2 (700 x 900),
orbfe_search_by_projection (1000 keypoints, 1000 queries, mode 1), orbfe_search_by_bow (two frames of 1000 features),
orbfe_keyframe_features_pack (1000), orbfe_vocabulary_transform (1000 features, levelsup 2) and orbfe_corner_subpix (64 corners of a
480 x 640 frame, window 4, 12 iterations, eps 0.005), 200 timings each through the ctypes binding.  ORBFE_LIB selects the library, so two builds can be run alternately; prints one JSON line."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from orb_slam2_aruco_amd import binding, synth

REPS = int(os.environ.get("REPS", "200"))
rng = np.random.default_rng(0)
frames = synth.stream(480, 640, 2, 1000)
ex = binding.ORBextractor(1000, 1.2, 8, 20, 7)
(k1, d1), (k2, d2) = ex(frames[0]), ex(frames[1])
k1, d1, k2, d2 = k1[:1000], d1[:1000], k2[:1000], d2[:1000]

# a complete k = 10, L = 3 tree of random descriptors (as tools/bow_timing.py builds its larger one)
k, Lv = 10, 3
counts = [k ** l for l in range(1, Lv + 1)]
nn = sum(counts)
parent = np.zeros(nn, np.int32); is_leaf = np.zeros(nn, np.uint8)
start, prev_start = 0, -1
for l, c in enumerate(counts):
    ids = np.arange(start, start + c)
    parent[start:start + c] = 0 if l == 0 else (prev_start + 1 + (ids - start) // k)
    if l == Lv - 1:
        is_leaf[start:start + c] = 1
    prev_start, start = start, start + c
voc = binding.ORBVocabulary.from_arrays(k, Lv, 0, 0, parent, is_leaf, rng.integers(0, 256, (nn, 32), dtype=np.uint8),
                                        np.where(is_leaf > 0, rng.uniform(0.5, 9.0, nn), 0.0))
fv1, fv2 = voc.transform(d1, 2)["fv"], voc.transform(d2, 2)["fv"]

# queries near the frame's keypoints, as projected map points are
pick = rng.integers(0, len(k1), 1000)
q = np.zeros(1000, binding.WINDOW_QUERY_DTYPE)
q["x"] = k1["x"][pick] + rng.normal(0, 2, 1000).astype(np.float32); q["y"] = k1["y"][pick] + rng.normal(0, 2, 1000).astype(np.float32)
q["r"] = (4.0 * 1.2 ** k1["octave"][pick]).astype(np.float32); q["min_level"] = k1["octave"][pick] - 1; q["max_level"] = k1["octave"][pick]
qd = d1[pick]
taken = (rng.random(len(k1)) < 0.15).astype(np.uint8)
corners = np.stack([k1["x"][:64], k1["y"][:64]], 1).astype(np.float32)
Q = rng.integers(0, 256, (700, 32), dtype=np.uint8); T = rng.integers(0, 256, (900, 32), dtype=np.uint8)

calls = {
    "orbfe_knn2": lambda: binding.knn2(Q, T),
    "orbfe_search_by_projection": lambda: binding.search_by_projection(k1, d1, 640, 480, q, qd, taken, 1, 100, 0.8),
    "orbfe_search_by_bow": lambda: binding.search_by_bow(k1, d1, fv1, k2, d2, fv2),
    "orbfe_keyframe_features_pack": lambda: binding.keyframe_features_pack(k1, d1),
    "orbfe_vocabulary_transform": lambda: voc.transform(d1, 2),
    "orbfe_corner_subpix": lambda: binding.corner_subpix(frames[0], corners, 4, 12, 0.005),
}
out = {"lib": binding.LIB_PATH, "reps": REPS, "n1": len(k1), "n2": len(k2)}
for name, call in calls.items():
    for _ in range(20):
        call()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    out[name + "_us"] = round(float(np.median(t)) * 1e6, 1)
print(json.dumps(out))
