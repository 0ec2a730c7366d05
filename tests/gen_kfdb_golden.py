"""Writes tests/golden/kfdb_cases.npz: what the REFERENCE's own KeyFrameDatabase returns on every case of tests/kfdb_cases.py and on the
script and the culling program of tests/kfdb_shim_driver.cpp.  Run by hand where the reference tree exists (REF, default /root/reference); no test calls it.

The reference's src/KeyFrameDatabase.cc, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp, BowVector.cpp and FeatureVector.cpp are compiled where they lie,
unchanged, into a temporary directory, against the mock headers of tests/mock_orbslam/ (KeyFrame.h, Frame.h, ORBVocabulary.h,
KeyFrameDatabase.h; the reference's real DBoW2 comes before the tree's stand-ins dbow2/) and with tests/kfdb_shim_driver.cpp as the program.  The mock KeyFrame starts its two scores from the case's
state.  What the reference shows from outside is recorded as it is: the candidates, every keyframe's score after the call, and
every keyframe's word count where its query field says it entered the sharing list.  Of the record, n_sharing, max / min common
words, n_scored and n_candidates follow from those; n_kept, best_acc_score and min_score_to_retain are locals of the reference that
no caller can see: they are the restatement's (tests/kfdb_ref.cpp), written only after the restatement has agreed with the reference
on everything else.  "extra" holds the restatement's counts that the coverage test reads (retained entries, entries whose best
keyframe is another one, stale contributions, kept scores equal to min_score)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
REF = os.environ.get("REF", "/root/reference")


def build_reference_driver(tmp):
    dbow2 = os.path.join(REF, "Thirdparty", "DBoW2", "DBoW2")
    exe = os.path.join(tmp, "kfdb_reference_driver")
    common = ["g++", "-O3", "-std=c++11", "-DKFDB_REFERENCE", "-I", REF, "-I", os.path.join(HERE, "mock_orbslam")]
    objs = []
    for src, extra in ((os.path.join(HERE, "kfdb_shim_driver.cpp"), []), (os.path.join(HERE, "mock_orbslam", "Frame_statics.cc"), []),
                       (os.path.join(REF, "src", "KeyFrameDatabase.cc"), []),
                       (os.path.join(dbow2, "BowVector.cpp"), []), (os.path.join(dbow2, "FeatureVector.cpp"), []),   # the mock KeyFrame holds both
                       (os.path.join(dbow2, "ScoringObject.cpp"),
                        ["-D__D_T_TEMPLATED_VOCABULARY__", "-include", "cmath", "-include", os.path.join(dbow2, "ScoringObject.h")])):
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.check_call(common + extra + ["-c", src, "-o", obj])
        objs.append(obj)
    subprocess.check_call(["g++"] + objs + ["-o", exe, "-pthread"])
    return exe


def dump_cases(path, cases):
    with open(path, "wb") as fh:
        fh.write(np.int32(len(cases)).tobytes())
        for c in cases:
            act = c["active"]
            fh.write(np.int32([c["mode"], c["K"], len(c["q_word"]), len(c["word"]), len(c["connected"]), act is not None]).tobytes())
            for a in (c["q_word"], c["q_value"], c["offsets"], c["word"], c["value"]) + ((act,) if act is not None else ()) + \
                    (c["neigh"], c["connected"], np.float32([c["min_score"]]), c["scores"]):
                fh.write(np.ascontiguousarray(a).tobytes())


def main():
    if not os.path.isfile(os.path.join(REF, "src", "KeyFrameDatabase.cc")):
        print("gen_kfdb_golden: no reference tree at %s; nothing written" % REF)
        return 0
    import kfdb_build as B
    import kfdb_cases as S
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference_driver(tmp)
        cases = [S.case(n) for n in S.CASES]
        dump = os.path.join(tmp, "kfdb_cases.dump")
        dump_cases(dump, cases)
        lines = subprocess.check_output([exe, "case", dump], text=True).split("\n")
        out["shim_script"] = np.array(subprocess.check_output([exe, "script"], text=True))
        out["shim_cull"] = np.array(subprocess.check_output([exe, "cull"], text=True))
    for i, (name, c) in enumerate(zip(S.CASES, cases)):
        head, sc, wd = lines[3 * i].split(), lines[3 * i + 1].split(), lines[3 * i + 2].split()
        assert head[0] == "case" and int(head[1]) == i and sc[0] == "scores" and wd[0] == "words", name
        cand = np.array([int(x) for x in head[3:]], np.int32)
        assert len(cand) == int(head[2])
        scores = np.array([int(x, 16) for x in sc[1:]], np.uint32)
        words = np.array([int(x) for x in wd[1:]], np.int32)
        r = B.detect(c)
        rec = r["result"].copy()
        # the reference, seen from outside
        sharing = words > 0
        maxc = int(words.max()) if sharing.any() else 0
        minc = int(np.float32(maxc) * np.float32(0.8))
        seen = dict(n_sharing=int(sharing.sum()), max_common_words=maxc, min_common_words=minc, n_scored=int((words > minc).sum()) if sharing.any() else 0,
                    n_candidates=len(cand))
        for k, v in seen.items():
            assert rec[k] == v, (name, k, rec[k], v)
        assert np.array_equal(r["candidates"], cand), (name, r["candidates"], cand)
        assert np.array_equal(r["scores"].view(np.uint32), scores), name
        assert np.array_equal(r["common"], words), name
        out[name + "/candidates"] = cand
        out[name + "/scores"] = scores
        out[name + "/common"] = words
        out[name + "/record"] = np.array([rec])
        out[name + "/extra"] = r["extra"]
        out[name + "/digest"] = S.digest(c)
    path = os.path.join(HERE, "golden", "kfdb_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
