"""GPU: include/shims/KeyFrameDatabase_orbfe.cc drives a mock map of 40 keyframes (+ 10 of a second map) through add, erase, clear,
both candidate queries and repeated relocalization queries (tests/kfdb_shim_driver.cpp, "script") and returns the KeyFrame ids the
reference's own KeyFrameDatabase.cc returned for the same program, in the same order (recorded in tests/golden/kfdb_cases.npz by
tests/gen_kfdb_golden.py)."""
import os
import subprocess

import numpy as np
import pytest

import shim_build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_returns_the_reference_keyframes_in_order(tmp_path):
    want = str(np.load(os.path.join(ROOT, "tests", "golden", "kfdb_cases.npz"))["shim_script"])
    lines = want.strip().split("\n")
    assert len(lines) == 10 and lines[7] == "reloc f3 empty:" and lines[6] == "loop kf39 high:"  # clear() and a min_score nothing reaches
    assert sum(len(l.split(":")[1].split()) >= 1 for l in lines) >= 6 and lines[0] != lines[2]    # erase() changed the repeated query
    exe = shim_build.build("kfdb", str(tmp_path))
    got = subprocess.run([exe, "script"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout == want


def test_shim_survives_keyframe_culling_beyond_the_bound_of_one_call(tmp_path):
    """9000 add() calls, all but the last 30 keyframes erased again: the erased positions are squeezed out, so the database the
    library sees stays far below ORBFE_KFDB_MAX_KEYFRAMES, and the three queries on the way return the reference's keyframes"""
    want = str(np.load(os.path.join(ROOT, "tests", "golden", "kfdb_cases.npz"))["shim_cull"])
    lines = want.strip().split("\n")
    assert len(lines) == 3 and all(len(l.split(":")[1].split()) >= 1 for l in lines)
    exe = shim_build.build("kfdb", str(tmp_path))
    got = subprocess.run([exe, "cull"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert got.returncode == 0, got.stderr
    assert got.stdout == want
