"""The matcher's plans (csrc/match_plan.hpp), compiled with g++ and run without a GPU: which knn2 kernel runs on how many splits of
the train set and on what grids, the buffers and arrays of SearchForInitialization, the LDS of the projection search as its launcher
sizes it and its kernel carves it, the growth rules of the overflow-and-repeat contract, the result block of the fuse batch.  The
literals are the rules of knn2_launch, sfi_launch and sbp_launch as they stood before the header existed, worked out by hand.  The same
driver, built as a program of its own with AddressSanitizer and UBSan, runs the knn2 sweep and writes every array of every layout."""
import subprocess

import pytest

import match_plan_build as mp

ERR_INVALID, ERR_CAPACITY = -1, -4   # include/orbfe.h


def test_constants():
    c = mp.constants()
    assert c == {"KNN_TILE": 256, "KM_WAVES": 8, "KM_CHUNK": 128, "SFI_MAXL0": 1024, "SFI_CURSOR_PAD": 64, "GRID_COLS": 64, "GRID_ROWS": 48,
                 "SBP_CELLS": 64 * 48, "MATCH_LDS_LIMIT": 150 * 1024}
    # the matrix-core kernel's workgroup covers the query tile of the VALU and the merge kernel: one x dimension for every grid
    assert c["KM_WAVES"] * 32 == c["KNN_TILE"]


# ---- knn2

# max_nq, max_nt, npairs, knn2_path -> mfma, nsplit, chunk, scan grid (None: not pinned)
KNN2_CASES = [
    (1000, 1000, 1, 0, 1, 8, 128, (4, 1, 8)),
    (1000, 1000, 1, 1, 0, 4, 256, (4, 1, 4)),
    (300, 128, 1, 0, 1, 1, 128, None),
    (300, 129, 1, 0, 1, 2, 128, None),      # the second split holds one descriptor
    (256, 1000, 600, 0, 1, 1, 1024, None),
    (256, 1000, 600, 1, 0, 2, 512, None),
]


@pytest.mark.parametrize("nq,nt,npairs,path,mfma,nsplit,chunk,scan", KNN2_CASES)
def test_knn2_plan(nq, nt, npairs, path, mfma, nsplit, chunk, scan):
    p = mp.knn2(nq, nt, npairs, 256, path)
    qtiles = (nq + 255) // 256
    assert (p["mfma"], p["nsplit"], p["chunk"]) == (mfma, nsplit, chunk)
    assert p["scan"] == (scan or (qtiles, npairs, nsplit))
    assert p["scan_block"] == (512 if mfma else 256)
    if nsplit > 1:
        assert p["merge"] == (qtiles, npairs) and p["part_bytes"] == npairs * nsplit * nq * 4
    else:
        assert p["merge"] is None and p["part_bytes"] == 0


def test_knn2_kernel_choice():
    # 0 and 2: the matrix cores wherever they apply; 1: never
    assert [mp.knn2(1000, 1000, 1, 256, path)["mfma"] for path in (0, 1, 2)] == [1, 0, 1]
    # they do not apply without a finite `init` ...
    assert [mp.knn2(1000, 1000, 1, 0, path)["mfma"] for path in (0, 1, 2)] == [0, 0, 0]
    # ... nor to a train index beyond 16 bits
    assert mp.knn2(1000, 65535, 1)["mfma"] == 1
    assert [mp.knn2(1000, 65536, 1, 256, path)["mfma"] for path in (0, 1, 2)] == [0, 0, 0]


def test_knn2_empty_train_set():
    for npairs in (1, 600, 2000):
        p = mp.knn2(300, 0, npairs)
        assert (p["mfma"], p["nsplit"], p["chunk"], p["merge"]) == (1, 1, 128, None)
        p = mp.knn2(300, 0, npairs, path=1)
        assert (p["mfma"], p["nsplit"], p["chunk"], p["merge"]) == (0, 1, 256, None)


def test_knn2_splits_cover_the_train_set_once():
    n = 0
    for nq in (1, 255, 256, 257, 1000, 5000):
        for nt in (0, 1, 127, 128, 129, 255, 256, 257, 1000, 5000, 65535, 65536):
            for npairs in (1, 2, 7, 64, 511, 512, 513, 1024, 1025):
                for path in (0, 1, 2):
                    p = mp.knn2(nq, nt, npairs, 256, path)
                    what = (nq, nt, npairs, path, p)
                    assert p["nsplit"] * p["chunk"] >= nt, what
                    assert p["nsplit"] == 1 or (p["nsplit"] - 1) * p["chunk"] < nt, what
                    assert p["chunk"] > 0 and p["chunk"] % (128 if p["mfma"] else 256) == 0, what
                    assert p["scan"] == ((nq + 255) // 256, npairs, p["nsplit"]), what
                    assert p["merge"] == (((nq + 255) // 256, npairs) if p["nsplit"] > 1 else None), what
                    n += 1
    assert mp.knn2_sweep() == (n, 0)   # the driver's own loop, which the sanitizer program runs


# ---- SearchForInitialization

SFI_ARRAYS = (("desc", 32), ("xy", 8), ("sorted", 4), ("qxy", 8), ("ang", 4), ("query", 2))   # element bytes per keypoint; 16-byte loads of desc
SFI_ALIGN = {"desc": 16, "xy": 8, "sorted": 4, "qxy": 8, "ang": 4, "query": 2}


def test_sfi_fresh_workspace_one_pair():
    l = mp.sfi(1, 0)
    assert (l["nframes"], l["pool"]) == (2, 16384)
    assert (l["cnt_bytes"], l["idx_bytes"], l["dist_bytes"], l["scratch_bytes"]) == (592, 119040, 66048, 4096)
    assert (l["nl0"], l["nq"], l["cursor"]) == (0, 2, 4)
    F = 2 * 1024
    assert [l[a] for a, _ in SFI_ARRAYS] == [0, 32 * F, 40 * F, 44 * F, 52 * F, 56 * F]


@pytest.mark.parametrize("npairs", [1, 2, 7, 64])
def test_sfi_arrays_are_aligned_disjoint_and_inside(npairs):
    l = mp.sfi(npairs, 0)
    F = (npairs + 1) * 1024
    end = 0
    for a, bytes_each in SFI_ARRAYS:
        assert l[a] >= end and l[a] % SFI_ALIGN[a] == 0, a
        end = l[a] + F * bytes_each
    assert end <= l["idx_bytes"]
    # nl0 | nq | a cursor per pair, 256 bytes apart
    assert l["nq"] >= l["nl0"] + npairs + 1 and l["cursor"] >= l["nq"] + npairs + 1
    assert (l["cursor"] + (npairs - 1) * 64 + 1) * 4 <= l["cnt_bytes"]
    # k_sfi_accept prefetches up to 63 entries past the last pool
    assert l["dist_bytes"] >= (npairs * l["pool"] + 63) * 4
    assert l["scratch_bytes"] == npairs * 1024 * 4


def test_sfi_pool_rules():
    assert mp.sfi(1, 0)["pool"] == 16384 and mp.sfi(1, 16384)["pool"] == 16384
    assert mp.sfi(1, 16385)["pool"] == 16388          # a multiple of 4
    assert mp.sfi_pool_after(16384, 90000) == 90112   # the next multiple of 1024
    assert mp.sfi_pool_after(16384, 16384) == 16384 and mp.sfi_pool_after(16384, 0) == 16384
    assert mp.sfi(3, 90112)["pool"] == 90112 and mp.sfi(3, 90112)["dist_bytes"] == 3 * 90112 * 4 + 512


@pytest.mark.parametrize("flags,need,err,pool,clear", [((0, 0), 0, 0, 16384, 0), ((0, 90000), 90000, 0, 90112, 1),
                                                       ((1100, 0), 1100, ERR_CAPACITY, 16384, 1), ((1100, 90000), 1100, ERR_CAPACITY, 90112, 1),
                                                       ((1024, 0), 0, 0, 16384, 1)])
def test_sfi_flag_rule(flags, need, err, pool, clear):
    assert mp.sfi_flags(flags[0], flags[1], 16384) == {"need": need, "err": err, "pool": pool, "clear": clear}


# ---- the projection searches

def test_sbp_capacity_1000():
    l = mp.sbp(1000)
    assert (l["err"], l["ncap"], l["lds_bytes"]) == (0, 1024, 20548)
    assert [l["lds_" + f] for f in ("sorted", "xy", "cell0", "lvl", "taken")] == [0, 4096, 12288, 18436, 19460]
    assert {f: l["lds_" + f] for f in mp.LDS_FIELDS} == mp.sbp_lds_offsets(1024)   # the kernel's call gives the launcher's carving


def test_sbp_lds_holds_its_arrays():
    ncap = 64
    while ncap <= 8192:
        o = mp.sbp_lds_offsets(ncap)
        l = mp.sbp(ncap)
        assert l["err"] == 0 and l["ncap"] == ncap
        # uint32 sorted[ncap] | float2 xy[ncap] | uint16 cell0[SBP_CELLS + 2] | uint8 lvl[ncap] | uint8 taken[ncap]
        assert o["sorted"] == 0 and o["xy"] >= o["sorted"] + 4 * ncap and o["cell0"] >= o["xy"] + 8 * ncap
        assert o["lvl"] >= o["cell0"] + 2 * (64 * 48 + 1) and o["taken"] >= o["lvl"] + ncap
        assert o["xy"] % 8 == 0 and o["cell0"] % 2 == 0
        assert o["taken"] + ncap <= o["end"] <= l["lds_bytes"] <= 150 * 1024
        ncap *= 2


def test_sbp_ncap_is_the_next_power_of_two_from_64():
    assert [mp.sbp(c)["ncap"] for c in (1, 64, 65, 1000, 1024, 1025, 8192)] == [64, 64, 128, 1024, 1024, 2048, 8192]


def test_sbp_refusals():
    assert mp.sbp(8192)["err"] == 0
    l = mp.sbp(8193)
    assert l["err"] == ERR_CAPACITY and "8193 keypoints do not fit" in l["msg"]
    assert mp.sbp(65535)["err"] == ERR_CAPACITY
    l = mp.sbp(65536)
    assert l["err"] == ERR_INVALID and "65535" in l["msg"]


def test_sbp_stride_rules():
    l = mp.sbp(1000, qcapacity=300, nframes=5, stride_now=0)
    assert l["stride"] == 128
    assert (l["rank_bytes"], l["dist_bytes"], l["cnt_bytes"]) == (1500 * 128 * 2, 1500 * 128, 1500 * 4)
    assert mp.sbp_stride_after(128, 600) == 640 and mp.sbp_stride_after(128, 100) == 128 and mp.sbp_stride_after(128, 0) == 128
    assert mp.sbp_stride_after(640, 640) == 640 and mp.sbp_stride_after(640, 641) == 704
    assert mp.sbp(1000, 300, 5, 640)["stride"] == 640 and mp.sbp(1000, 300, 5, 640)["rank_bytes"] == 1500 * 640 * 2


# ---- the fuse batch

def test_fuse_batch_layout():
    nkf, nmp = 3, 500
    NQ = nkf * nmp
    l = mp.fuse_batch(nkf, nmp)
    assert l["q_bytes"] == NQ * 20   # sizeof(orbfe_window_query)
    parts = [(l[a], NQ) for a in ("best_level", "second_dist", "second_level", "match")] + [(l["nq"], nkf), (l["nmatches"], nkf)]
    end = 0
    for off, n in parts:   # in ints, in this order, without overlap
        assert off >= end
        end = off + n
    assert end * 4 <= l["obest_bytes"]
    assert l["nq"] == 4 * NQ and l["nmatches"] == 4 * NQ + nkf


def test_plans_under_sanitizers():
    exe = mp.sanitizer_program()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "1944 plans, 0 violations" in r.stdout and "layouts: 0 bytes claimed twice" in r.stdout, r.stdout
