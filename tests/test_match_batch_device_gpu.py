"""The matcher's batched device entry points on their own terms: ragged batches (frames of 0, 1, 63, 64, 65, capacity, 200 and 2
keypoints, poison behind every frame's valid rows, guard bytes around every output) and the overflow-and-repeat contract of the
status calls.  Every value is compared bit for bit with the oracle and, where one exists, with the per-frame host-pointer entry
point.  In-process through the library's own allocator (pose_opt_device.Dev), on the null stream; the overflow tests run in a thread
of their own, whose workspace starts at the smallest row stride (128) and candidate pool (16 384 per pair)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import match_batch_cases as mc
import oracle_lib as oracle
from orb_slam2_aruco_amd import binding as orbfe
from pose_opt_device import Dev, Out

pytestmark = pytest.mark.gpu

SEED = 7
P32 = mc.POISON_I32
ORBFE_ERR_CAPACITY = orbfe.ORBFE_ERR_CAPACITY


def i32(*shape):
    return Out(np.full(shape, P32, np.int32))


def lib():
    return orbfe.load()


def ok(rc):
    assert rc == 0, lib().orbfe_last_error().decode()


def cp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def in_fresh_thread(fn):
    """fn() in a thread of its own: the library's per-thread workspaces start empty there"""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001
            box["error"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def sbp_status():
    v = C.c_int32(-1)
    return lib().orbfe_search_by_projection_batch_status(None, C.byref(v)), v.value


def sfi_status():
    v = C.c_int32(-1)
    return lib().orbfe_search_for_initialization_batch_status(None, C.byref(v)), v.value


def same_bytes(a, b):
    """equal as bytes (records with NaN poison compare equal to themselves)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class DevCase:
    """the input blocks of a packed batch on the device"""

    def __init__(self, case):
        self.case, self.cap, self.F = case, case["capacity"], len(case["n"])
        self.kps, self.desc, self.n = Dev(case["kps"]), Dev(case["desc"]), Dev(case["n"])
        # the same counts with every full frame but the last claiming capacity + 5, for the entry points whose header promises
        # min(d_n[f], capacity).  The five records behind such a block are the next frame's: in the projection searches, Fuse and the
        # vocabulary transform a missing clamp changes results; in the bag-of-words and triangulation searches the feature vectors
        # come from a transform that has clamped already, so there only the number of match12 / match21 entries written is tested
        over = case["n"].copy()
        over[:-1][over[:-1] == self.cap] += 5
        self.n_over = Dev(over)


@functools.lru_cache(maxsize=None)
def ragged():
    return mc.ragged_frames(SEED)


@pytest.fixture(scope="module")
def dev_rag():
    """the ragged batch on the device, shared by the tests of this module and freed with it"""
    return DevCase(ragged())


# ---------------------------------------------------------------------------------------------------- 1. knn2
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("init", [256, 60, 2**31 - 1])
def test_knn2_batch_device(path, init):
    Q, T = mc.knn2_pairs(SEED)
    nq = np.array([len(q) for q in Q], np.int32); nt = np.array([len(t) for t in T], np.int32)
    max_nq, max_nt = int(nq.max()), int(nt.max())
    q_stride, t_stride = max_nq * 32 + 96, max_nt * 32 + 64           # gaps between the blocks, poisoned
    dQ, dnq, dnt = Dev(mc.pack_rows(Q, max_nq, q_stride)), Dev(nq), Dev(nt)
    dT = Dev(mc.pack_rows(T, max_nt, t_stride)); dTs = Dev(mc.pack_rows([T[6]], max_nt, t_stride))
    orbfe.debug_control("knn2_path", path)
    try:
        for shared in (False, True):                                     # t_stride = 0: one train block for every pair
            outs = [i32(8, max_nq) for _ in range(3)]
            ok(lib().orbfe_knn2_batch_device(dQ.ptr, dnq.ptr, q_stride, max_nq, (dTs if shared else dT).ptr, dnt.ptr, 0 if shared else t_stride,
                                             max_nt, 8, init, outs[0].ptr, outs[1].ptr, outs[2].ptr, None))
            got = [o.get() for o in outs]
            for p in range(8):
                Tp = T[6][:nt[p]] if shared else T[p]
                want = oracle.knn2(Q[p], Tp, init)
                host = orbfe.knn2(Q[p], Tp, init) if nq[p] else want
                for g, w, h, name in zip(got, want, host, ("best_idx", "best_dist", "second_dist")):
                    assert np.array_equal(g[p, :nq[p]], w), (shared, p, name)
                    assert np.array_equal(h, w), (shared, p, name, "host")
                    assert np.all(g[p, nq[p]:] == P32), (shared, p, name, "rows past nq")
    finally:
        orbfe.debug_control("knn2_path", 0)


# ---------------------------------------------------------------------------------------------------- 2 - 4. SearchForInitialization
def sfi_call(dc, npairs, bounds, window, ori, m12, nm):
    ok(lib().orbfe_search_for_initialization_batch_device(dc.kps.ptr, dc.desc.ptr, dc.n.ptr, dc.cap, npairs, mc.COLS, mc.ROWS, cp(bounds), window,
                                                         0.9, ori, m12.ptr, nm.ptr, None))


def sfi_check_pair(case, p, m12, nm, want, what=""):
    n1 = case["n"][p]
    assert nm[p] == want[0], (p, what, int(nm[p]), want[0])
    assert np.array_equal(m12[p, :n1], want[1]), (p, what)
    assert np.all(m12[p, n1:] == P32), (p, what, "rows past n")


@pytest.mark.parametrize("ori", [1, 0])
@pytest.mark.parametrize("bounds", [None, mc.DISTORTED_BOUNDS], ids=["plain", "distorted"])
def test_search_for_initialization_batch_device(ori, bounds):
    case = mc.reorder(ragged(), list(range(8)) + [0])                    # the empty frame is F1 of pair 0 and F2 of pair 7
    dc = DevCase(case)
    m12, nm = i32(8, dc.cap), i32(8)
    sfi_call(dc, 8, bounds, 100, ori, m12, nm)
    assert sfi_status() == (0, 0)
    gm, gn = m12.get(), nm.get()
    matcher = orbfe.ORBmatcher(0.9, bool(ori))
    for p in range(8):
        (k1, d1), (k2, d2) = case["frames"][p], case["frames"][p + 1]
        want = oracle.search_for_initialization(k1, d1, k2, d2, mc.COLS, mc.ROWS, None, 100, 0.9, bool(ori), bounds)
        sfi_check_pair(case, p, gm, gn, want)
        if len(k1) and len(k2):
            hn, hm, _ = matcher.SearchForInitialization(k1, d1, k2, d2, mc.COLS, mc.ROWS, None, 100, bounds=bounds)
            assert hn == want[0] and np.array_equal(hm, want[1]), (p, "host")


def test_search_for_initialization_batch_overflow_and_repeat():
    """Pair 1 needs 90 000 pool entries against the 16 384 of a fresh workspace: the status call reports what the pair needed and
    grows the pool, the same batch repeated unchanged is complete.  The neighbours' pools are their own: pairs 0 and 2 are right on
    the first attempt already."""
    case = mc.sfi_overflow_case()
    want = [oracle.search_for_initialization(*case["frames"][p], *case["frames"][p + 1], mc.COLS, mc.ROWS, None, 100, 0.9, True) for p in range(3)]
    need = mc.sfi_candidates(case["frames"][1][0], case["frames"][2][0], 100)

    def run():
        dc = DevCase(case)
        m12, nm = i32(3, dc.cap), i32(3)
        sfi_call(dc, 3, None, 100, 1, m12, nm)
        st1 = sfi_status()
        first = (m12.get(), nm.get())
        sfi_call(dc, 3, None, 100, 1, m12, nm)
        st2 = sfi_status()
        return st1, first, st2, (m12.get(), nm.get())
    st1, first, st2, second = in_fresh_thread(run)
    print("SearchForInitialization overflow: status", st1, "oracle candidates", need, "then", st2)
    assert st1[0] == 0 and st1[1] >= need and st1[1] > 16384, (st1, need)
    for p in (0, 2):
        sfi_check_pair(case, p, *first, want[p], "first attempt")
    assert st2 == (0, 0)
    for p in range(3):
        sfi_check_pair(case, p, *second, want[p], "repeat")


def test_search_for_initialization_batch_capacity_limit():
    """1100 level-0 keypoints in frame 2: ORBFE_ERR_CAPACITY with the count; reading clears the flag; pairs 0 and 3 are untouched"""
    case = mc.sfi_capacity_case()

    def run():
        dc = DevCase(case)
        m12, nm = i32(4, dc.cap), i32(4)
        sfi_call(dc, 4, None, 10, 1, m12, nm)
        return sfi_status(), sfi_status(), m12.get(), nm.get()
    st1, st2, gm, gn = in_fresh_thread(run)
    assert st1 == (ORBFE_ERR_CAPACITY, 1100), st1
    assert st2 == (0, 0), st2
    for p in (0, 3):
        want = oracle.search_for_initialization(*case["frames"][p], *case["frames"][p + 1], mc.COLS, mc.ROWS, None, 10, 0.9, True)
        assert want[0] > 0
        sfi_check_pair(case, p, gm, gn, want)
    for p in (1, 2):
        assert np.all(gm[p, case["n"][p]:] == P32)


def test_search_for_initialization_batch_capacity_limit_with_a_pool_overflow():
    """The 1100-keypoint frame and a pair that needs 90 000 pool entries in one batch: the status call still answers
    ORBFE_ERR_CAPACITY with the level-0 count, and it has grown the pool -- a following batch that needs the same 90 000 entries
    (the overflow case, without the big frame) is complete at once, with no overflow to report."""
    both, follow = mc.sfi_capacity_and_pool_case(), mc.sfi_overflow_case()
    want = [oracle.search_for_initialization(*follow["frames"][p], *follow["frames"][p + 1], mc.COLS, mc.ROWS, None, 100, 0.9, True) for p in range(3)]

    def run():
        dc = DevCase(both)
        m12, nm = i32(4, dc.cap), i32(4)
        sfi_call(dc, 4, None, 100, 1, m12, nm)
        st1 = sfi_status()
        m12.get(); nm.get()                                              # guards
        dc2 = DevCase(follow)
        m12b, nmb = i32(3, dc2.cap), i32(3)
        sfi_call(dc2, 3, None, 100, 1, m12b, nmb)
        return st1, sfi_status(), m12b.get(), nmb.get()
    st1, st2, gm, gn = in_fresh_thread(run)
    assert st1 == (ORBFE_ERR_CAPACITY, 1100), st1
    assert st2 == (0, 0), st2
    for p in range(3):
        sfi_check_pair(follow, p, gm, gn, want[p])


# ---------------------------------------------------------------------------------------------------- 5 - 7. projection searches
RAW = ("best_idx", "best_dist", "best_level", "second_dist", "second_level")


class SbpBuffers:
    def __init__(self, dc, qs, use_taken=True):
        self.dc, self.qs, self.QC = dc, qs, qs["qcapacity"]
        self.q, self.qd, self.nq = Dev(qs["q"]), Dev(qs["qdesc"]), Dev(qs["nq"])
        self.qobs, self.qang = Dev(qs["qobs"]), Dev(qs["qang"])
        self.taken0 = qs["taken"].copy()
        for f in range(dc.F):
            self.taken0[f, dc.case["n"][f]:] = 0x5A                     # flags behind the valid rows: poison
        self.taken = Out(self.taken0) if use_taken else None
        self.raw = [i32(dc.F, self.QC) for _ in range(5)]
        self.match, self.match_cur, self.nm = i32(dc.F, self.QC), i32(dc.F, dc.cap), i32(dc.F)

    def call(self, mode, bounds=None, ori=1):
        dc = self.dc
        ok(lib().orbfe_search_by_projection_batch_device(dc.kps.ptr, dc.desc.ptr, dc.n_over.ptr, dc.cap, dc.F, mc.COLS, mc.ROWS, cp(bounds), self.q.ptr,
                                                        self.qd.ptr, self.nq.ptr, self.QC, self.taken.ptr if self.taken else None, self.qobs.ptr,
                                                        self.qang.ptr, mode, 100, 0.8, 1.0 / 30, ori, *[o.ptr for o in self.raw], self.match.ptr,
                                                        self.match_cur.ptr, self.nm.ptr, None))

    def get(self):
        return dict(raw=[o.get() for o in self.raw], match=self.match.get(), match_cur=self.match_cur.get(), nm=self.nm.get(),
                    taken=self.taken.get() if self.taken else None)

    def check_frame(self, got, f, mode, bounds=None, ori=1, what=""):
        """frame f of a finished call against the oracle and the host-pointer entry point; poison behind nq resp. n"""
        case, qs = self.dc.case, self.qs
        k, d = case["frames"][f]
        n, m = len(k), int(qs["nq"][f])
        q, qd, qobs, qang = qs["q"][f, :m], qs["qdesc"][f, :m], qs["qobs"][f, :m], qs["qang"][f, :m]
        tk = qs["taken"][f, :n] if self.taken else None
        tag = (what, mode, f)
        for j in range(5):
            assert np.all(got["raw"][j][f, m:] == P32), tag + (RAW[j], "rows past nq")
        assert np.all(got["match"][f, m:] == P32) and np.all(got["match_cur"][f, n:] == P32), tag
        if self.taken:
            assert np.all(got["taken"][f, n:] == 0x5A), tag + ("taken flags past n",)
        if mode < 2:
            want = oracle.search_by_projection(k, d, mc.COLS, mc.ROWS, q, qd, tk, mode, 100, 0.8, bounds, q_observed=qobs)
            host = orbfe.search_by_projection(k, d, mc.COLS, mc.ROWS, q, qd, tk, mode, 100, 0.8, bounds=bounds, q_observed=qobs)
            for j, name in enumerate(RAW):
                assert np.array_equal(got["raw"][j][f, :m], want[name]), tag + (name,)
                assert np.array_equal(host[name], want[name]), tag + (name, "host")
            if mode == 0:   # documented: mode 0 writes neither d_match nor d_nmatches
                assert np.all(got["match"][f] == P32) and got["nm"][f] == P32 and np.all(got["match_cur"][f] == P32), tag
                if self.taken:
                    assert np.array_equal(got["taken"][f, :n], tk), tag
            else:
                assert got["nm"][f] == want["nmatches"] == host["nmatches"], tag
                assert np.array_equal(got["match"][f, :m], want["match"]) and np.array_equal(host["match"], want["match"]), tag
                if self.taken:
                    assert np.array_equal(got["taken"][f, :n], want["taken"]) and np.array_equal(host["taken"], want["taken"]), tag
            if n == 0 and m > 0:
                assert np.all(got["raw"][0][f, :m] == -1) and np.all(got["raw"][1][f, :m] == 256) and np.all(got["raw"][3][f, :m] == 256), tag
                assert np.all(got["raw"][2][f, :m] == -1) and np.all(got["raw"][4][f, :m] == -1), tag
            return want["nmatches"] if mode else int((want["best_idx"] >= 0).sum())
        # mode 2: the best-only loop restated over the oracle's per-query search (match_batch_cases.best_only_reference), and the
        # host-pointer entry point, which returns match_cur and the count
        want = mc.best_only_reference(k, d, q, qd, qobs, qang, tk, ori, bounds)
        hn, hm = orbfe.search_by_projection_best(k, d, mc.COLS, mc.ROWS, q, qang, qd, 100, 1.0 / 30, q_blocks=qobs, taken=tk,
                                                 check_orientation=bool(ori), bounds=bounds)
        assert got["nm"][f] == want["nmatches"] == hn, tag
        assert np.array_equal(got["match_cur"][f, :n], want["match_cur"]) and np.array_equal(hm, want["match_cur"]), tag
        assert np.array_equal(got["match"][f, :m], want["match"]), tag
        for j, name in enumerate(RAW):       # each query's best / second-best among the keypoints not taken when its turn came
            assert np.array_equal(got["raw"][j][f, :m], want["raw"][j]), tag + (name,)
        if self.taken:
            assert np.array_equal(got["taken"][f, :n], want["taken"]), tag + ("taken flags",)
        # and the relations between the outputs themselves
        mt = got["match"][f, :m]
        acc = got["raw"][1][f, :m] <= 100
        assert np.array_equal(mt, np.where(acc, got["raw"][0][f, :m], -1)), tag
        held = np.flatnonzero(got["match_cur"][f, :n] >= 0)
        assert np.array_equal(mt[got["match_cur"][f, held]], held), tag
        if n == 0 and m > 0:
            assert np.all(mt == -1) and np.all(got["raw"][0][f, :m] == -1) and np.all(got["raw"][1][f, :m] == 256), tag
        return want["nmatches"]


@pytest.mark.parametrize("mode,use_taken,ori", [(0, False, 1), (0, True, 1), (1, False, 1), (1, True, 1), (2, False, 1), (2, True, 1),
                                                (2, False, 0), (2, True, 0)])
def test_search_by_projection_batch_device(dev_rag, mode, use_taken, ori):
    dc = dev_rag
    qs = mc.projection_queries(ragged(), SEED + 1, 200)
    bounds = mc.DISTORTED_BOUNDS if use_taken else None
    b = SbpBuffers(dc, qs, use_taken)
    b.call(mode, bounds, ori)
    assert sbp_status() == (0, 0)
    got = b.get()
    found = [b.check_frame(got, f, mode, bounds, ori) for f in range(dc.F)]
    assert all(found[f] > 0 for f in (2, 3, 4, 5)), found


def test_search_by_projection_batch_overflow_and_repeat():
    """Frame 3's one window holds 600 candidates against a row stride of 128: the status call says 600 and grows the stride; truncation
    is silent and the first attempt has marked keypoints, so the caller uploads its taken flags again and repeats.  The other four
    frames are right on the first attempt."""
    case, qs = mc.projection_overflow_case(SEED)

    def run():
        b = SbpBuffers(DevCase(case), qs)
        b.call(1)
        st1 = sbp_status()
        first = b.get()
        b.taken.put(b.taken0)
        b.call(1)
        st2 = sbp_status()
        return b, st1, first, st2, b.get()
    b, st1, first, st2, second = in_fresh_thread(run)
    assert st1 == (0, 600), st1
    for f in (0, 1, 2, 4):
        b.check_frame(first, f, 1, what="first attempt")
    assert st2 == (0, 0), st2
    for f in range(5):
        b.check_frame(second, f, 1, what="repeat")
    assert second["nm"][3] == 1


def test_search_by_projection_batch_overflow_flag_is_sticky():
    """two batches before one status read: the first overflows, the second does not -- the flag is still set, and read once"""
    case, qs = mc.projection_overflow_case(SEED)
    rqs = mc.projection_queries(ragged(), SEED + 1, 200)

    def run():
        a, b = SbpBuffers(DevCase(case), qs), SbpBuffers(DevCase(ragged()), rqs)
        a.call(1)
        b.call(1)
        st = [sbp_status(), sbp_status()]
        return b, st, b.get()
    b, st, got = in_fresh_thread(run)
    assert st == [(0, 600), (0, 0)], st
    for f in range(8):
        b.check_frame(got, f, 1)                                         # the batch that did not overflow is complete


# ---------------------------------------------------------------------------------------------------- 8. Fuse
@pytest.mark.parametrize("chi2", [5.99, 0.0])
@pytest.mark.parametrize("use_valid", [False, True])
def test_fuse_search_batch_device(dev_rag, chi2, use_valid):
    dc, case = dev_rag, ragged()
    fc = mc.fuse_case(case, SEED + 2)
    sf, _, isg, logsf = mc.scale_tables()
    nmp = fc["nmp"]
    ins = [Dev(fc[k]) for k in ("x3", "valid", "min_d", "max_d", "nrm", "mp_desc")]
    bi, bd = i32(8, nmp), i32(8, nmp)
    ok(lib().orbfe_fuse_search_batch_device(dc.kps.ptr, dc.desc.ptr, dc.n_over.ptr, dc.cap, 8, mc.COLS, mc.ROWS, None, ins[0].ptr,
                                           ins[1].ptr if use_valid else None, ins[2].ptr, ins[3].ptr, ins[4].ptr, ins[5].ptr, nmp, cp(fc["Tcw"]),
                                           cp(fc["Ow"]), cp(mc.TUM1_K), cp(sf), cp(isg), 8, logsf, 3.0, chi2, bi.ptr, bd.ptr, None))
    assert sbp_status() == (0, 0)
    gi, gd = bi.get(), bd.get()
    for k in range(8):
        kk, dd = case["frames"][k]
        args = (kk, dd, mc.COLS, mc.ROWS, fc["x3"], fc["valid"][k] if use_valid else None, fc["min_d"], fc["max_d"], fc["nrm"], fc["mp_desc"],
                fc["Tcw"][k].reshape(3, 4), fc["Ow"][k], mc.TUM1_K, sf, isg, logsf, 3.0, chi2)
        want = oracle.fuse_search(*args)
        assert np.array_equal(gi[k], want[0]) and np.array_equal(gd[k], want[1]), (k, chi2)
        if len(kk):
            host = orbfe.fuse_search(*args)
            assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1]), (k, "host")
        else:
            assert np.all(gi[k] == -1) and np.all(gd[k] == 256)
        if len(kk) >= 63:
            assert (gd[k] <= 50).sum() > 0, k


# ---------------------------------------------------------------------------------------------------- 9. vocabulary transform
U32_POISON, F64_POISON = np.uint32(0xDEADBEEF), np.float64(-7777.0)


@pytest.fixture(scope="module")
def vocs():
    voc, ovoc = mc.vocabulary(SEED + 3)
    return ovoc, orbfe.ORBVocabulary.from_arrays(10, 4, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])


@pytest.fixture(scope="module", params=[1, 4], ids=["levelsup1", "levelsup4"])
def transformed(request, dev_rag, vocs):
    """The ragged batch through orbfe_vocabulary_transform_batch_device at one levelsup: (levelsup, the output buffers, the oracle's
    vectors).  The vocabulary test checks the buffers; the bag-of-words and triangulation tests take them as their input."""
    dc, levelsup = dev_rag, request.param
    ovoc, gvoc = vocs
    F, cap = dc.F, dc.cap
    o = dict(word=i32(F, cap), node=i32(F, cap), weight=Out(np.full((F, cap), F64_POISON)), bw=Out(np.full((F, cap), U32_POISON)),
             bv=Out(np.full((F, cap), F64_POISON)), nb=i32(F), fn=Out(np.full((F, cap), U32_POISON)), fo=i32(F, cap + 1),
             ff=Out(np.full((F, cap), U32_POISON)), nf=i32(F))
    ok(lib().orbfe_vocabulary_transform_batch_device(gvoc.h, dc.desc.ptr, dc.n_over.ptr, cap, F, levelsup, *[o[k].ptr for k in
                                                    ("word", "node", "weight", "bw", "bv", "nb", "fn", "fo", "ff", "nf")], None))
    return levelsup, o, [ovoc.transform(d, levelsup) for _, d in ragged()["frames"]]


def test_vocabulary_transform_batch_device(transformed, vocs):
    levelsup, o, want = transformed
    g = {k: v.get() for k, v in o.items()}
    _, gvoc = vocs
    u64 = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for f, (_, d) in enumerate(ragged()["frames"]):
        w, n = want[f], len(d)
        nb, nf = int(g["nb"][f]), int(g["nf"][f])
        assert nb == len(w["bow"][0]) and nf == len(w["fv"][0]), f
        assert np.array_equal(g["word"][f, :n], w["word"]) and np.array_equal(g["node"][f, :n], w["node"]), f
        assert np.array_equal(u64(g["weight"][f, :n]), u64(w["weight"])), f
        assert np.array_equal(g["bw"][f, :nb], w["bow"][0]) and np.array_equal(u64(g["bv"][f, :nb]), u64(w["bow"][1])), f
        assert np.array_equal(g["fn"][f, :nf], w["fv"][0]) and np.array_equal(g["fo"][f, :nf + 1], w["fv"][1]), f
        assert np.array_equal(g["ff"][f, :g["fo"][f, nf]], w["fv"][2]), f
        # behind the valid rows every block keeps its poison
        assert np.all(g["word"][f, n:] == P32) and np.all(g["node"][f, n:] == P32) and np.all(g["weight"][f, n:] == F64_POISON), f
        assert np.all(g["bw"][f, nb:] == U32_POISON) and np.all(g["bv"][f, nb:] == F64_POISON), f
        assert np.all(g["fn"][f, nf:] == U32_POISON) and np.all(g["fo"][f, nf + 1:] == P32) and np.all(g["ff"][f, g["fo"][f, nf]:] == U32_POISON), f
        if n == 0:
            assert nb == 0 and nf == 0 and g["fo"][f, 0] == 0
        else:
            h = gvoc.transform(d, levelsup)
            assert np.array_equal(u64(h["bow"][1]), u64(w["bow"][1])) and all(np.array_equal(a, b) for a, b in zip(h["fv"], w["fv"])), (f, "host")
    assert any((w["weight"] == 0).any() for w in want)                   # stop words were hit


# ---------------------------------------------------------------------------------------------------- 10. SearchByBoW, SearchForTriangulation
def pair_arrays(explicit):
    pairs = mc.BOW_PAIRS if explicit else [(p, p + 1) for p in range(7)]
    if not explicit:
        return pairs, None, None
    return pairs, Dev(np.array([a for a, _ in pairs], np.int32)), Dev(np.array([b for _, b in pairs], np.int32))


def flags(period):
    """per-keypoint flags [F][capacity]: 0 for every period-th valid row, poison behind n"""
    case = ragged()
    v = np.full((8, case["capacity"]), 0x5A, np.uint8)
    for f, n in enumerate(case["n"]):
        v[f, :n] = np.arange(n) % period != 0
    return v


@pytest.mark.parametrize("explicit", [True, False], ids=["pair_arrays", "null_pairs"])
@pytest.mark.parametrize("kfkf", [False, True], ids=["kf_frame", "kf_kf"])
def test_search_by_bow_batch_device(dev_rag, transformed, explicit, kfkf):
    dc, case = dev_rag, ragged()
    _, o, tr = transformed
    pairs, dp1, dp2 = pair_arrays(explicit)
    valid = flags(7)
    dvalid = Dev(valid)
    amax, factor = (49, 1.0 / 30) if kfkf else (50, 30 / 360.0)
    m12, m21, nm = i32(len(pairs), dc.cap), i32(len(pairs), dc.cap), i32(len(pairs))
    ok(lib().orbfe_search_by_bow_batch_device(dc.kps.ptr, dc.desc.ptr, dvalid.ptr, dc.n_over.ptr, o["fn"].ptr, o["fo"].ptr, o["ff"].ptr, o["nf"].ptr, dc.cap,
                                             dp1.ptr if dp1 else None, dp2.ptr if dp2 else None, len(pairs), int(kfkf), 0.7, 1, amax, factor,
                                             m12.ptr, m21.ptr, nm.ptr, None))
    g12, g21, gn = m12.get(), m21.get(), nm.get()
    for p, (a, b) in enumerate(pairs):
        (ka, da), (kb, db) = case["frames"][a], case["frames"][b]
        args = (ka, da, tr[a]["fv"], kb, db, tr[b]["fv"], valid[a, :len(ka)], valid[b, :len(kb)] if kfkf else None, 0.7, True, amax, factor)
        wn, w12, w21 = oracle.search_by_bow(*args)
        assert gn[p] == wn and np.array_equal(g12[p, :len(ka)], w12) and np.array_equal(g21[p, :len(kb)], w21), (p, a, b)
        assert np.all(g12[p, len(ka):] == P32) and np.all(g21[p, len(kb):] == P32), (p, "rows past n")
        if len(ka) and len(kb):
            hn, h12, h21 = orbfe.search_by_bow(*args)
            assert hn == wn and np.array_equal(h12, w12) and np.array_equal(h21, w21), (p, "host")
        if len(ka) >= 63 and len(kb) >= 63:
            assert wn > 0, (a, b)
    if explicit:   # the repeated pair (6, 5): the same blocks twice
        assert np.array_equal(g12[1], g12[6]) and np.array_equal(g21[1], g21[6]) and gn[1] == gn[6]


@pytest.mark.parametrize("explicit", [True, False], ids=["pair_arrays", "null_pairs"])
@pytest.mark.parametrize("use_free", [False, True])
def test_search_for_triangulation_batch_device(dev_rag, transformed, explicit, use_free):
    dc, case = dev_rag, ragged()
    _, o, tr = transformed
    pairs, dp1, dp2 = pair_arrays(explicit)
    free = flags(5)
    dfree = Dev(free)
    F12, epi = mc.triangulation_geometry(len(pairs))
    dF, de = Dev(F12), Dev(epi)
    sf, sg, _, _ = mc.scale_tables()
    m12, s21, nm = i32(len(pairs), dc.cap), i32(len(pairs), dc.cap), i32(len(pairs))
    ok(lib().orbfe_search_for_triangulation_batch_device(dc.kps.ptr, dc.desc.ptr, dfree.ptr if use_free else None, dc.n_over.ptr, o["fn"].ptr, o["fo"].ptr,
                                                        o["ff"].ptr, o["nf"].ptr, dc.cap, dp1.ptr if dp1 else None, dp2.ptr if dp2 else None,
                                                        len(pairs), dF.ptr, de.ptr, cp(sf), cp(sg), 8, 1, m12.ptr, s21.ptr, nm.ptr, None))
    g12, gn = m12.get(), nm.get()
    s21.get()                                                            # guards of the scratch block
    for p, (a, b) in enumerate(pairs):
        (ka, da), (kb, db) = case["frames"][a], case["frames"][b]
        has1 = 1 - free[a, :len(ka)] if use_free else None
        has2 = 1 - free[b, :len(kb)] if use_free else None
        args = (ka, da, tr[a]["fv"], kb, db, tr[b]["fv"], F12[p].reshape(3, 3), epi[p], sf, sg, has1, has2)
        wn, w12 = oracle.search_for_triangulation(*args)
        assert gn[p] == wn and np.array_equal(g12[p, :len(ka)], w12), (p, a, b)
        assert np.all(g12[p, len(ka):] == P32), (p, "rows past n")
        if len(ka) and len(kb):
            hn, h12 = orbfe.search_for_triangulation(*args)
            assert hn == wn and np.array_equal(h12, w12), (p, "host")
        if p == 2:
            assert wn == 0                                               # the all-zero F12
        elif len(ka) >= 63 and len(kb) >= 63:
            assert wn > 0, (a, b)
    if explicit:
        assert not np.array_equal(F12[1], F12[6])                        # the repeated pair has another F12: geometry is per pair, not per frame


# ---------------------------------------------------------------------------------------------------- 11. undistortion
@pytest.mark.parametrize("ndist", [0, 4, 5, 8])
@pytest.mark.parametrize("in_place", [False, True])
def test_undistort_keypoints_batch_device(ndist, in_place):
    case = ragged()
    cap = case["capacity"]
    dist = np.concatenate([mc.TUM1_DIST, [0.01, -0.02, 0.005]]).astype(np.float32)[:ndist]
    n_dev = case["n"].copy(); n_dev[5] = cap + 5                         # the header promises min(d_n[f], capacity)
    dn = Dev(n_dev)
    src = Out(case["kps"])
    dst_poison = np.frombuffer(bytes([0x6B]) * (8 * cap * mc.KP_DTYPE.itemsize), mc.KP_DTYPE).reshape(8, cap)
    dst = src if in_place else Out(dst_poison)
    ok(lib().orbfe_undistort_keypoints_batch_device(src.ptr, dn.ptr, cap, 8, cp(mc.TUM1_K), cp(dist) if ndist else None, ndist, dst.ptr, None))
    got = dst.get()
    if not in_place:
        assert same_bytes(src.get(), case["kps"])                        # the source is only read
    for f, (k, _) in enumerate(case["frames"]):
        n = len(k)
        want = k.copy()
        if ndist and n:
            xy = oracle.undistort_points(np.stack([k["x"], k["y"]], 1), mc.TUM1_K, dist)
            want["x"] = xy[:, 0]; want["y"] = xy[:, 1]
            assert not np.array_equal(want["x"], k["x"])
            assert same_bytes(orbfe.UndistortKeyPoints(k, mc.TUM1_K, dist), want), (f, "host")
        assert same_bytes(got[f, :n], want), f
        # behind the valid rows: untouched -- except that the copy of ndist == 0 is of whole blocks (documented)
        behind = case["kps"][f, n:] if in_place or ndist == 0 else dst_poison[f, n:]
        assert same_bytes(got[f, n:], behind), (f, "rows past n")


# ---------------------------------------------------------------------------------------------------- 12. distinctive descriptors
def distinctive_call(desc, offsets, want_desc):
    npoints = len(offsets) - 1
    dd, do = Dev(desc), Dev(offsets)
    bi = i32(npoints)
    bdesc = Out(np.full((npoints, 32), 0x5A, np.uint8)) if want_desc else None
    ok(lib().orbfe_distinctive_descriptors_device(dd.ptr, do.ptr, npoints, bi.ptr, bdesc.ptr if bdesc else None, None))
    return bi.get(), bdesc.get() if bdesc else None


@pytest.mark.parametrize("want_desc", [False, True])
def test_distinctive_descriptors_device(want_desc):
    rng = np.random.default_rng(11)
    sizes = mc.DISTINCTIVE_SIZES + rng.integers(1, 40, 400).tolist()
    rng.shuffle(sizes)
    assert len(sizes) % 4 == 1
    desc, off = mc.distinctive_case(11, sizes)
    want = oracle.distinctive_descriptors(desc, off)
    got, chosen = distinctive_call(desc, off, want_desc)
    assert np.array_equal(got, want)
    host, hdesc = orbfe.distinctive_descriptors(desc, off)
    assert np.array_equal(host, want)
    if want_desc:
        for p, n in enumerate(sizes):
            assert np.array_equal(chosen[p], desc[off[p] + got[p]] if n else np.full(32, 0x5A, np.uint8)), p
    # one point of 300 observations among the others: the device call cannot refuse it and answers from its first 256 rows
    at = len(sizes) // 2
    sizes2 = sizes[:at] + [300] + sizes[at:]
    desc2, off2 = mc.distinctive_case(12, sizes2)
    others = np.delete(np.arange(len(sizes2)), at)
    want2 = oracle.distinctive_descriptors(np.concatenate([desc2[:off2[at]], desc2[off2[at + 1]:]]), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    first256 = oracle.distinctive_descriptors(desc2[off2[at]:off2[at] + 256], np.array([0, 256], np.int32))[0]
    got2, chosen2 = distinctive_call(desc2, off2, want_desc)
    assert np.array_equal(got2[others], want2)
    assert 0 <= got2[at] < 256 and got2[at] == first256
    if want_desc:
        assert np.array_equal(chosen2[at], desc2[off2[at] + first256])
