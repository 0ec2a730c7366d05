"""CPU tests of the collect step of include/shims/Optimizer_essential_orbfe.cc on the hand-built mock map of
tests/essential_shim_driver.cpp (its head says what the map holds and why), and of the program that links every shim."""
import subprocess

import numpy as np
import pytest

import essential_shim_build as B
import shim_build


@pytest.fixture(scope="module")
def collected(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("eg_shim"))
    return B.run(B.build_driver(out), "collect", out)


def test_vertices_are_the_keyframes_that_are_not_bad(collected):
    d = collected
    assert d["vk"].tolist() == [0, 1, 2, 3, 4, 6, 7] and d["id"].tolist() == [10, 12, 14, 16, 18, 22, 24]
    assert d["fixed"].tolist() == [1]                       # the loop keyframe, in the middle of the order
    assert d["cpos"].tolist() == [5, 6] and d["npos"].tolist() == [5, 6]   # keyframe 6 is corrected and not fixed
    assert d["threw"].tolist() == [1]
    assert d["Tcw"].shape == (7 * 12,) and d["csim"].shape == (16,) and np.all(d["csim"].reshape(2, 8)[:, 7] == 1.0)
    assert not np.array_equal(d["csim"], d["nsim"]) and np.array_equal(d["csim"].reshape(2, 8)[:, :4], d["nsim"].reshape(2, 8)[:, :4])


def test_edges_follow_the_reference_rules_in_insertion_order(collected):
    d = collected
    edges = list(zip(d["ei"].tolist(), d["ej"].tolist(), d["ek"].tolist()))
    loop, normal = [e for e in edges if e[2] == 0], [e for e in edges if e[2] == 1]
    assert edges == loop + normal                           # LoopConnections first
    # (7, 1) with weight 30 survives as the cur / loop pair, (7, 2) with 50 does not; (6, 2) with 150 does.  The map of
    # LoopConnections is ordered by pointer, which the test does not fix: either keyframe's group may come first
    assert sorted(loop) == [(5, 2, 0), (6, 1, 0)]
    assert normal == [(1, 0, 1), (2, 1, 1), (2, 0, 1), (3, 2, 1), (3, 1, 1), (4, 3, 1),
                      (4, 0, 1),                            # the old loop edge, from the larger id, before the covisibles
                      (4, 2, 1), (5, 4, 1), (6, 5, 1)]
    assert (5, 2, 1) not in edges                           # loop connection and covisible: kept once
    assert all(i != j for i, j, _ in edges)


def test_point_references(collected):
    # 6 is bad; 7 goes through mnCorrectedReference (keyframe 6, position 5); 11's reference keyframe is bad
    assert collected["pref"].tolist() == [0, 2, 3, 4, 5, 6, -1, 5, 2, 3, 3, -1]
    assert collected["x"].shape == (36,)


def test_all_shims_link_into_one_program(tmp_path):
    exe = shim_build.build("all", str(tmp_path))
    assert subprocess.check_output([exe], text=True).strip() == "ok: 11 shims in one program"
