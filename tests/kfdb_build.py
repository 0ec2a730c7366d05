"""Builds tests/kfdb_ref.cpp (the CPU restatement of KeyFrameDatabase's candidate queries and DBoW2's L1 score) with g++ and loads it
with ctypes (test infrastructure, in the manner of tests/sim3_opt_build.py).  One build per process, in a temporary directory."""
import ctypes as C

import numpy as np

import ref_build

_lib = None

RESULT_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common_words", "<i4"), ("min_common_words", "<i4"), ("n_scored", "<i4"),
                         ("n_kept", "<i4"), ("n_candidates", "<i4"), ("best_acc_score", "<f4"), ("min_score_to_retain", "<f4"),
                         ("status", "<i4")])
LOOP, RELOC = 0, 1
# the restatement's extra counts (tests/kfdb_ref.cpp)
N_RETAINED, N_BEST_OTHER, N_STALE, N_KEPT_EQ_MIN = 0, 1, 2, 3


def lib():
    global _lib
    if _lib is None:
        L = ref_build.build_shared("kfdb_ref.cpp")
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        L.kfdb_score.argtypes = [vp, vp, i32, vp, vp, i32]
        L.kfdb_score.restype = C.c_double
        L.kfdb_min_score.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp, i32]
        L.kfdb_min_score.restype = f32
        L.kfdb_detect.argtypes = [i32, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, f32, vp, vp, vp, vp, vp, vp]
        L.kfdb_detect.restype = i32
        L.kfdb_open.argtypes = [vp, vp, vp, vp, i32, vp]
        L.kfdb_open.restype = vp
        L.kfdb_close.argtypes = [vp]
        L.kfdb_close.restype = None
        L.kfdb_query.argtypes = [vp, i32, vp, vp, i32, vp, i32, f32, vp, vp, vp, vp, vp, vp]
        L.kfdb_query.restype = i32
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Database:
    """The restatement's database of a case, built once and queried many times (tools/kfdb_timing.py clocks query() alone, as the
    reference holds its inverted file ready)."""

    def __init__(self, c):
        self.K = c["K"]
        self.h = lib().kfdb_open(_p(c["offsets"]), _p(c["word"]), _p(c["value"]), _p(c["active"]), c["K"], _p(c["neigh"]))

    def query(self, c, scores):
        """one query of case c (its mode, query vector, connected list and min_score) on the state array `scores`, updated in place"""
        K = self.K
        cand, common = np.full(max(K, 1), -1, np.int32), np.zeros(max(K, 1), np.int32)
        res, extra, order = np.zeros(1, RESULT_DTYPE), np.zeros(4, np.int32), np.zeros(max(K, 1), np.int32)
        lib().kfdb_query(self.h, c["mode"], _p(c["q_word"]), _p(c["q_value"]), len(c["q_word"]), _p(c["connected"]), len(c["connected"]),
                         float(c["min_score"]), _p(scores), _p(cand), _p(common), _p(res), _p(extra), _p(order))
        return dict(candidates=cand[:res[0]["n_candidates"]].copy(), common=common[:K], result=res[0], scores=scores, extra=extra,
                    order=order[:res[0]["n_sharing"]].copy())

    def __del__(self):
        if getattr(self, "h", None):
            lib().kfdb_close(self.h)
            self.h = None


def score(w1, v1, w2, v2):
    """L1Scoring::score as a double"""
    w1, w2 = np.ascontiguousarray(w1, np.uint32), np.ascontiguousarray(w2, np.uint32)
    v1, v2 = np.ascontiguousarray(v1, np.float64), np.ascontiguousarray(v2, np.float64)
    return lib().kfdb_score(_p(w1), _p(v1), len(w1), _p(w2), _p(v2), len(w2))


def min_score(c):
    """DetectLoop's minScore of a case (a dict of tests/kfdb_cases.py)"""
    return np.float32(lib().kfdb_min_score(_p(c["q_word"]), _p(c["q_value"]), len(c["q_word"]), _p(c["offsets"]), _p(c["word"]), _p(c["value"]),
                                           _p(c["active"]), c["K"], _p(c["connected"]), len(c["connected"])))


def detect(c, scores=None, min_score=None):
    """The restatement on one case.  Returns dict(candidates, common, result record, scores (the state after the call), extra,
    order (the sharing list))."""
    K = c["K"]
    sc = np.array(c["scores"] if scores is None else scores, np.float32)
    cand, common = np.full(max(K, 1), -1, np.int32), np.zeros(max(K, 1), np.int32)
    res, extra, order = np.zeros(1, RESULT_DTYPE), np.zeros(4, np.int32), np.zeros(max(K, 1), np.int32)
    rc = lib().kfdb_detect(c["mode"], _p(c["q_word"]), _p(c["q_value"]), len(c["q_word"]), _p(c["offsets"]), _p(c["word"]), _p(c["value"]),
                           _p(c["active"]), K, _p(c["neigh"]), _p(c["connected"]), len(c["connected"]),
                           float(c["min_score"] if min_score is None else min_score), _p(sc), _p(cand), _p(common), _p(res), _p(extra), _p(order))
    assert rc == 0
    return dict(candidates=cand[:res[0]["n_candidates"]].copy(), common=common[:K], result=res[0], scores=sc, extra=extra,
                order=order[:res[0]["n_sharing"]].copy())
