"""Host-side builders of the cases the matcher's batched device entry points are tested on (tests/test_match_batch_device_gpu.py), and
the CPU proof that they are not vacuous (tests/test_match_batch_cases_cpu.py).  numpy and the oracle only: nothing here touches a GPU.

A batch is a set of per-frame blocks of `capacity` records.  Rows from n[f] to capacity hold a recognisable poison -- keypoint fields
NaN / -1, descriptor bytes 0xA5 -- so that a kernel which reads them computes visibly wrong results and one which writes them is caught."""
import numpy as np

import oracle_lib as oracle

KP_DTYPE = oracle.KP_DTYPE
WQ_DTYPE = oracle.WINDOW_QUERY_DTYPE
COLS, ROWS = 640, 480
CAPACITY = 384
COUNTS = [0, 1, 63, 64, 65, 384, 200, 2]
POISON_DESC = 0xA5
POISON_I32 = -7777                       # fill of the int32 outputs: no entry point produces it
# TUM1.yaml of the reference (Examples/Monocular/TUM1.yaml)
TUM1_K = np.array([517.306408, 516.469215, 318.643040, 255.313989], np.float32)
TUM1_DIST = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)
DISTORTED_BOUNDS = np.array([-14.25, -9.5, 655.75, 489.0], np.float32)   # the undistorted image of a distorted camera reaches beyond the sensor


def patch_keypoints(rng, dtype, n, x0, y0, side, octaves=1):
    """n keypoints scattered over the square patch of `side` pixels at (x0, y0)"""
    k = np.zeros(n, dtype)
    k["x"] = x0 + rng.random(n, dtype=np.float32) * side
    k["y"] = y0 + rng.random(n, dtype=np.float32) * side
    k["size"] = 31.0; k["angle"] = rng.random(n, dtype=np.float32) * 360.0; k["response"] = 50.0
    k["octave"] = rng.integers(0, octaves, n); k["class_id"] = -1
    return k


def flip_bits(rng, desc, most):
    d = desc.copy()
    for i in range(len(d)):
        for b in rng.integers(0, 256, 8)[: rng.integers(0, most + 1)]:
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def poison_keypoints(n):
    k = np.zeros(n, KP_DTYPE)
    for name in KP_DTYPE.names:
        k[name] = np.nan if KP_DTYPE[name].kind == "f" else -1
    return k


def poison_queries(n):
    q = np.zeros(n, WQ_DTYPE)
    q["x"] = np.nan; q["y"] = np.nan; q["r"] = np.nan; q["min_level"] = -1; q["max_level"] = -1
    return q


def pack(frames, capacity):
    """[(keypoints, descriptors)] -> dict(kps [F][capacity], desc [F][capacity][32], n [F], capacity, frames), poisoned past n[f]"""
    F = len(frames)
    kps = np.tile(poison_keypoints(capacity), (F, 1))
    desc = np.full((F, capacity, 32), POISON_DESC, np.uint8)
    n = np.zeros(F, np.int32)
    for f, (k, d) in enumerate(frames):
        assert len(k) == len(d) <= capacity
        n[f] = len(k); kps[f, :len(k)] = k; desc[f, :len(k)] = d
    return dict(kps=kps, desc=desc, n=n, capacity=capacity, frames=[(k.copy(), d.copy()) for k, d in frames])


def ragged_frames(seed):
    """F = 8 frames of 0, 1, 63, 64, 65, 384 (= capacity), 200 and 2 keypoints over 640 x 480, octaves 0 .. 7 (the lower ones more
    often, as an extractor gives them).  All frames observe one scene of 384 points whose descriptors are clustered (24 centres, 48
    bits of spread): frame f sees the first n[f] of them, in an order of its own, each moved by a pixel or two, turned by a few
    degrees and with at most 4 descriptor bits flipped -- so two frames' views of a point differ by at most 8 bits and real matches
    occur between any two frames, neighbours included, over min(n) common points."""
    rng = np.random.default_rng(seed)
    N = CAPACITY
    scene = np.zeros(N, KP_DTYPE)
    scene["x"] = rng.uniform(12.0, COLS - 12.0, N).astype(np.float32)
    scene["y"] = rng.uniform(12.0, ROWS - 12.0, N).astype(np.float32)
    p = 1.2 ** -np.arange(8.0)
    scene["octave"] = rng.choice(8, N, p=p / p.sum())
    scene["size"] = (31.0 * 1.2 ** scene["octave"]).astype(np.float32)
    scene["angle"] = rng.uniform(5.0, 355.0, N).astype(np.float32)
    scene["response"] = rng.uniform(20.0, 120.0, N).astype(np.float32)
    scene["class_id"] = -1
    centres = rng.integers(0, 256, (24, 32), dtype=np.uint8)
    sdesc = centres[rng.integers(0, 24, N)].copy()
    for i in range(N):
        for b in rng.choice(256, 48, replace=False):
            sdesc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    frames = []
    for n in COUNTS:
        ids = rng.permutation(n)
        k = scene[ids].copy()
        k["x"] += rng.normal(0, 1.5, n).astype(np.float32)
        k["y"] += rng.normal(0, 1.5, n).astype(np.float32)
        k["angle"] = (k["angle"] + rng.normal(0, 2.0, n)).astype(np.float32)
        frames.append((k, flip_bits(rng, sdesc[ids], 4)))
    return pack(frames, CAPACITY)


def reorder(case, order, capacity=None):
    """the batch made of the frames `order` of another"""
    return pack([case["frames"][f] for f in order], capacity or case["capacity"])


# ------------------------------------------------------------------------------------------------ knn2
def knn2_pairs(seed):
    """eight (Q, T) problems; nq == 0, nt == 0, nq == max_nq and nt == max_nt all occur; ties in best and in second planted"""
    nq = [0, 1, 63, 64, 65, 300, 17, 128]
    nt = [65, 0, 64, 63, 1, 140, 300, 5]
    rng = np.random.default_rng(seed)
    Q, T = [], []
    for a, b in zip(nq, nt):
        q = rng.integers(0, 256, (a, 32), dtype=np.uint8); t = rng.integers(0, 256, (b, 32), dtype=np.uint8)
        if b > 40:   # duplicates and near-duplicates: ties in best and in second
            t[7] = t[3]; t[40] = t[3]
            if a > 0: q[0] = t[3]
            if a > 2: q[2] = t[3] ^ np.uint8(1)
        Q.append(q); T.append(t)
    return Q, T


def pack_rows(blocks, rows, stride_bytes, row_bytes=32):
    """descriptor blocks `stride_bytes` apart, `rows` rows each; everything that is not a valid row is poison"""
    out = np.full((len(blocks), stride_bytes), POISON_DESC, np.uint8)
    for p, b in enumerate(blocks):
        assert len(b) <= rows and rows * row_bytes <= stride_bytes
        out[p, :len(b) * row_bytes] = b.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------ projection searches
def projection_queries(case, seed, qcapacity, r0=6.0):
    """Frame f is searched with queries built from frame (f + 1) % F's keypoints (as tests/device_pipeline_case.py does), at most
    qcapacity of them: with the ragged frames nq = 1, 63, 64, 65, qcapacity, qcapacity, 2, 0.  Rows past nq[f] are poison."""
    rng = np.random.default_rng(seed)
    F, cap = len(case["n"]), case["capacity"]
    q = np.tile(poison_queries(qcapacity), (F, 1))
    qd = np.full((F, qcapacity, 32), POISON_DESC, np.uint8)
    qobs = np.full((F, qcapacity), 1, np.uint8); qang = np.full((F, qcapacity), np.nan, np.float32)
    nq = np.zeros(F, np.int32)
    taken = np.zeros((F, cap), np.uint8)
    for f in range(F):
        ks, ds = case["frames"][(f + 1) % F]
        sel = rng.permutation(len(ks))[:qcapacity]
        m = nq[f] = len(sel)
        q["x"][f, :m] = ks["x"][sel] + rng.normal(0, 1.5, m).astype(np.float32)
        q["y"][f, :m] = ks["y"][sel] + rng.normal(0, 1.5, m).astype(np.float32)
        q["r"][f, :m] = (r0 * 1.2 ** ks["octave"][sel]).astype(np.float32)
        q["min_level"][f, :m] = ks["octave"][sel] - 1
        q["max_level"][f, :m] = ks["octave"][sel] + (f % 2)
        qd[f, :m] = ds[sel]; qang[f, :m] = ks["angle"][sel]
        qobs[f, :m] = rng.random(m) < 0.7
        taken[f, :case["n"][f]] = rng.random(case["n"][f]) < 0.1
    return dict(q=q, qdesc=qd, nq=nq, qobs=qobs, qang=qang, taken=taken, qcapacity=qcapacity)


def projection_overflow_case(seed):
    """Five frames; frame 3 is a patch of 600 keypoints inside 40 x 40 px with ONE window that covers it: a candidate row of 600
    against the 128 a fresh workspace holds.  The query's descriptor is that of the LAST free keypoint in candidate order, so a row
    cut at 128 does not hold the match.  The other four frames are ragged frames 2, 3, 4 and 6 with ordinary queries."""
    rng = np.random.default_rng(seed)
    rag = ragged_frames(seed)
    patch = patch_keypoints(rng, KP_DTYPE, 600, 300.0, 200.0, 40.0, octaves=8)
    pdesc = rng.integers(0, 256, (600, 32), dtype=np.uint8)
    frames = [rag["frames"][2], rag["frames"][3], rag["frames"][4], (patch, pdesc), rag["frames"][6]]
    case = pack(frames, 640)
    qs = projection_queries(case, seed + 1, 64)
    taken3 = (rng.random(600) < 0.3).astype(np.uint8)
    qs["nq"][3] = 1
    qs["q"][3, 0] = (320.0, 220.0, 50.0, 0, -1)
    _, order = oracle.features_in_area(patch, COLS, ROWS, [320.0], [220.0], 50.0, 0, -1)
    target = [i for i in order if not taken3[i]][-1]
    qs["qdesc"][3, 0] = flip_bits(rng, pdesc[target][None], 6)[0]
    qs["qobs"][3, 0] = 1
    qs["taken"][3] = 0; qs["taken"][3, :600] = taken3
    qs["q"][3, 1:] = poison_queries(63); qs["qdesc"][3, 1:] = POISON_DESC; qs["qang"][3, 1:] = np.nan
    return case, qs


def best_only_reference(k, d, q, qdesc, qobs, qang, taken, ori, bounds=None, th_high=100, factor=1.0 / 30):
    """Mode 2 of the projection searches (the best-only loop of ORBmatcher.cc:1332-1474 / :1476-1603 on caller-projected queries) from
    the oracle's per-query best / second-best: query by query, the best keypoint among those not taken yet is accepted when its
    distance is <= th_high, receives the query (a later query overwrites an earlier one) and is taken from then on if the query's
    map point is observed; then the rotation histogram over every accepted query and ComputeThreeMaxima (:1605-1646).
    -> dict(raw [5][nq], match [nq], match_cur [n], nmatches, taken [n])"""
    n, m = len(k), len(q)
    tk = np.zeros(n, np.uint8) if taken is None else np.ascontiguousarray(taken, np.uint8).copy()
    raw = np.zeros((5, m), np.int32); match = np.full(m, -1, np.int32); cur = np.full(n, -1, np.int32)
    bins = np.full(m, -1, np.int64)
    f32 = np.float32
    for i in range(m):
        r = oracle.search_by_projection(k, d, COLS, ROWS, q[i:i + 1], qdesc[i:i + 1], tk, 0, th_high, 0.8, bounds)
        for j, name in enumerate(("best_idx", "best_dist", "best_level", "second_dist", "second_level")):
            raw[j, i] = r[name][0]
        b = int(r["best_idx"][0])
        if b < 0 or r["best_dist"][0] > th_high:
            continue
        match[i] = b; cur[b] = i
        if qobs is None or qobs[i]:
            tk[b] = 1
        rot = f32(qang[i]) - f32(k["angle"][b])
        if rot < 0:
            rot = f32(rot + f32(360.0))
        bn = int(np.floor(np.float64(f32(rot * f32(factor))) + 0.5))     # roundf of a non-negative float
        bins[i] = min(max(0 if bn == 30 else bn, 0), 29)
    nm = int((match >= 0).sum())
    if ori:
        hist = np.bincount(bins[match >= 0], minlength=30)
        ind, mx = [-1, -1, -1], [0, 0, 0]
        for i, s in enumerate(hist):
            if s > mx[0]: mx, ind = [s, mx[0], mx[1]], [i, ind[0], ind[1]]
            elif s > mx[1]: mx, ind = [mx[0], s, mx[1]], [ind[0], i, ind[1]]
            elif s > mx[2]: mx[2], ind[2] = s, i
        if f32(mx[1]) < f32(0.1) * f32(mx[0]): ind[1] = ind[2] = -1
        elif f32(mx[2]) < f32(0.1) * f32(mx[0]): ind[2] = -1
        for i in np.flatnonzero(match >= 0):
            if bins[i] not in ind:
                cur[match[i]] = -1; nm -= 1
    return dict(raw=raw, match=match, match_cur=cur, nmatches=nm, taken=tk)


def longest_candidate_list(kps, q, bounds=None):
    """the longest list Frame::GetFeaturesInArea returns for the window queries q over the keypoints kps"""
    longest = 0
    for w in q:
        if not w["r"] >= 0:
            continue
        off, _ = oracle.features_in_area(kps, COLS, ROWS, [w["x"]], [w["y"]], float(w["r"]), int(w["min_level"]), int(w["max_level"]), bounds)
        longest = max(longest, int(off[1]))
    return longest


# ------------------------------------------------------------------------------------------------ SearchForInitialization
def sfi_candidates(k1, k2, window, bounds=None):
    """pool entries a pair needs: the candidates of F1's level-0 keypoints among F2's level-0 keypoints (ORBmatcher.cc:425-431)"""
    q = k1[k1["octave"] <= 0]
    if len(q) == 0 or len(k2) == 0:
        return 0
    off, _ = oracle.features_in_area(k2, COLS, ROWS, q["x"], q["y"], float(window), 0, 0, bounds)
    return int(off[-1])


def sfi_overflow_case(seed=22):
    """Four frames, three pairs; pair 1 is the 300-keypoint pair of test_search_for_initialization_retries_from_the_callers_prev_matched
    (level 0, one 60 x 60 px patch, window 100: 90 000 pool entries against the 16 384 of a fresh workspace).  Frame 0 sees 40 of
    frame 1's points and frame 3 sees 40 of frame 2's, so pairs 0 and 2 have matches and need 12 000 entries each."""
    rng = np.random.default_rng(seed)
    n = 300
    k1 = patch_keypoints(rng, KP_DTYPE, n, 280.0, 200.0, 60.0)
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)

    def view(k, d, count):
        ids = rng.permutation(len(k))[:count]
        kk = k[ids].copy()
        kk["x"] = np.clip(kk["x"] + rng.normal(0, 2, count).astype(np.float32), 280.0, 340.0)
        kk["y"] = np.clip(kk["y"] + rng.normal(0, 2, count).astype(np.float32), 200.0, 260.0)
        return kk, flip_bits(rng, d[ids], 8)
    k2, d2 = view(k1, d1, n)
    return pack([view(k1, d1, 40), (k1, d1), (k2, d2), view(k2, d2, 40)], 320)


def sfi_capacity_and_pool_case(seed=23):
    """The 1024 level-0 limit and a pool overflow in ONE batch: pair 0 is pair 1 of sfi_overflow_case (90 000 pool entries), frame 2
    the 1100-keypoint frame of sfi_capacity_case; searched at window 100."""
    ov, cp = sfi_overflow_case(), sfi_capacity_case(seed)
    return pack([ov["frames"][1], ov["frames"][2], cp["frames"][2], cp["frames"][3], cp["frames"][4]], 1104)


def sfi_capacity_case(seed=23):
    """Five frames; frame 2 has 1100 level-0 keypoints (the kernels hold 1024), the others are ragged frames 3, 4, 6 and 5.  Pairs 0
    and 3 do not touch frame 2.  Searched at window 10, where no pair comes near the pool size."""
    rng = np.random.default_rng(seed)
    rag = ragged_frames(seed)
    big = patch_keypoints(rng, KP_DTYPE, 1100, 20.0, 20.0, 440.0)
    bdesc = rng.integers(0, 256, (1100, 32), dtype=np.uint8)
    return pack([rag["frames"][3], rag["frames"][4], (big, bdesc), rag["frames"][6], rag["frames"][5]], 1104)


# ------------------------------------------------------------------------------------------------ Fuse
def scale_tables():
    sf = np.ones(8, np.float32)
    for l in range(1, 8):
        sf[l] = np.float32(sf[l - 1] * np.float32(1.2))
    return sf, (sf * sf).astype(np.float32), (1.0 / (sf * sf)).astype(np.float32), np.float32(np.log(np.float32(1.2)))


def fuse_case(case, seed, nmp=257, source=5):
    """nmp map points back-projected from the first nmp keypoints of frame `source`, shared by all keyframes of the batch, each under
    a pose of its own (small translations); valid is [nkf][nmp]"""
    rng = np.random.default_rng(seed)
    k0, d0 = case["frames"][source]
    k0, d0 = k0[:nmp], d0[:nmp]
    sf = scale_tables()[0]
    z = rng.uniform(2.0, 6.0, nmp).astype(np.float32)
    x3 = np.stack([(k0["x"] - TUM1_K[2]) / TUM1_K[0] * z, (k0["y"] - TUM1_K[3]) / TUM1_K[1] * z, z], 1).astype(np.float32)
    d3 = np.linalg.norm(x3, axis=1).astype(np.float32)
    max_d = (d3 * sf[k0["octave"]]).astype(np.float32)
    min_d = (max_d / sf[7]).astype(np.float32)
    nrm = (x3 / d3[:, None]).astype(np.float32)
    nkf = len(case["n"])
    Tcw = np.zeros((nkf, 12), np.float32); Ow = np.zeros((nkf, 3), np.float32)
    for k in range(nkf):
        T = np.eye(3, 4, dtype=np.float32); T[:, 3] = [0.004 * k, -0.002 * k, 0.002 * k]
        Tcw[k] = T.reshape(-1); Ow[k] = -T[:, 3]
    valid = (rng.random((nkf, nmp)) < 0.9).astype(np.uint8)
    return dict(x3=x3, min_d=min_d, max_d=max_d, nrm=nrm, mp_desc=np.ascontiguousarray(d0), Tcw=Tcw, Ow=Ow, valid=valid, nmp=nmp)


# ------------------------------------------------------------------------------------------------ vocabulary, pairs
BOW_PAIRS = [(5, 6), (6, 5), (5, 5), (0, 5), (5, 0), (1, 2), (6, 5)]   # a self-pair, an empty side on either side, tiny frames, a repeat


def vocabulary(seed):
    import voc_cases
    voc = voc_cases.make(10, 4, seed, irregular=True)
    return voc, oracle.VocabularyOracle.from_arrays(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])


def triangulation_geometry(npairs):
    """F12 and epipole per pair, all different; pair 2's F12 is all zero (no epipolar line: 0 matches).  The others are the F of a
    sideways translation (lines y2 = y1) with a growing vertical shear, so that the band test decides."""
    F12 = np.zeros((npairs, 9), np.float32); epi = np.zeros((npairs, 2), np.float32)
    for p in range(npairs):
        F12[p] = [0, 0, 0, 0, 0, -1, 0, 1, 0.25 * p]
        epi[p] = [-1e4 + 100.0 * p, 240.0]
    if npairs > 2:
        F12[2] = 0
    epi[0] = [320.0, 240.0]   # an epipole inside the image: the keypoints around it are dropped (:752-757)
    return F12, epi


# ------------------------------------------------------------------------------------------------ distinctive descriptors
def distinctive_case(seed, sizes):
    """CSR lists of observations: per point a base descriptor with up to 3 bits flipped per observation (ties in the medians)"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    desc = np.zeros((max(int(offsets[-1]), 1), 32), np.uint8)
    for p, n in enumerate(sizes):
        blk = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (n, 1))
        flips = rng.integers(0, 256, (n, 3))
        for i in range(n):
            for b in flips[i][:rng.integers(0, 4)]:
                blk[i, b >> 3] ^= np.uint8(1 << (b & 7))
        desc[offsets[p]:offsets[p + 1]] = blk
    return desc[:offsets[-1]], offsets


DISTINCTIVE_SIZES = [0, 1, 2, 3, 4, 5, 7, 16, 33, 63, 64, 65, 127, 128, 129, 200, 256]
